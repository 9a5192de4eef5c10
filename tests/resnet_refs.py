"""Operands and fp64 references of the ModifiedResNet tower's kernels (tests/test_gpu_resnet_blocks.py): torch's own conv2d /
avg_pool2d / indexing on the CPU in float64 -- none of them goes through the oracle's restatement of the tower.  Every case is built
once per process (lru_cache) and shared by the tests that need it; nothing writes to a cached tensor.

Layouts: activations NHWC; 3x3 weights as torch has them, [cout, cin, 3, 3], and `conv3_rows` is their [cout, 9 * cin] form in
(ky, kx, c) order that the kernel reads; stem weights [cout_pad, 3, 3, 3] = [cout_pad, 27] in (c, ky, kx) order as they are."""
import functools
import zlib

import torch
import torch.nn.functional as F


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))      # the same operands in every process


def conv3_rows(w4):
    """[cout, cin, 3, 3] -> [cout, 9 * cin], k = (ky * 3 + kx) * cin + c."""
    return w4.permute(0, 2, 3, 1).reshape(w4.shape[0], -1).contiguous()


def conv3_ref(x, w4, bias):
    """fp64 relu(conv3x3 stride 1 pad 1 + bias), NHWC in and out."""
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w4.double(), bias.double(), padding=1)
    return F.relu(y).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def conv3_case(b, H, W, cin, cout, integer=False):
    """(x [b,H,W,cin], w4 [cout,cin,3,3], bias [cout], fp64 reference).  integer: x in {-2..2}, w in {-1,0,1}, bias in {-3..3}:
    every partial sum is an integer below 2^24, so the fp32 result is exact whatever the order."""
    g = _gen("conv3", b, H, W, cin, cout, integer)
    if integer:
        x = torch.randint(-2, 3, (b, H, W, cin), generator=g).float()
        w4 = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).float()
        bias = torch.randint(-3, 4, (cout,), generator=g).float()
    else:
        x = torch.randn(b, H, W, cin, generator=g)
        w4 = torch.randn(cout, cin, 3, 3, generator=g) * (9 * cin) ** -0.5
        bias = torch.randn(cout, generator=g)
    return x, w4, bias, conv3_ref(x, w4, bias)


def tap_weights(cin, cout, ky, kx):
    """[cout, cin, 3, 3]: output channel c copies input channel c from tap (ky, kx) alone (c < min(cin, cout)); everything else is 0."""
    w4 = torch.zeros(cout, cin, 3, 3)
    c = torch.arange(min(cin, cout))
    w4[c, c, ky, kx] = 1.0
    return w4


def tap_shift(x, cout, ky, kx):
    """What tap_weights must give on x [b,H,W,cin] >= 0, by plain indexing: out[b,y,x,c] = x[b, y + ky - 1, x + kx - 1, c] inside the
    image, 0.0 outside it and in the channels past min(cin, cout)."""
    b, H, W, cin = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros(b, H, W, cout)
    n = min(cin, cout)
    out[..., :n] = xp[:, ky:ky + H, kx:kx + W, :n]
    return out


@functools.lru_cache(maxsize=None)
def conv1_case(M, N, K, integer=False):
    """(a [M,K], w [N,K], bias [N], residual [M,N], fp64 a w^T + bias)."""
    g = _gen("conv1", M, N, K, integer)
    if integer:
        a = torch.randint(-2, 3, (M, K), generator=g).float()
        w = torch.randint(-1, 2, (N, K), generator=g).float()
        bias = torch.randint(-3, 4, (N,), generator=g).float()
        r = torch.randint(-4, 5, (M, N), generator=g).float()
    else:
        a = torch.randn(M, K, generator=g)
        w = torch.randn(N, K, generator=g) * K ** -0.5
        bias = torch.randn(N, generator=g)
        r = torch.randn(M, N, generator=g)
    return a, w, bias, r, a.double() @ w.double().T + bias.double()


def stem_ref(img, w4, bias):
    """fp64 relu(conv3x3 stride 2 pad 1 + bias): NCHW image in, NHWC out."""
    y = F.conv2d(img.double(), w4.double(), bias.double(), stride=2, padding=1)
    return F.relu(y).permute(0, 2, 3, 1).contiguous()


def stem_zero_channels(cp):
    """The channels of a stem case whose weights and bias are zero: the tail, as the BatchNorm fold pads 40 -> 48."""
    return slice(cp - (8 if cp == 48 else 4), cp)


@functools.lru_cache(maxsize=None)
def stem_case(b, S, cp, integer=False):
    """(img [b,3,S,S], w4 [cp,3,3,3], bias [cp], fp64 reference); the channels of stem_zero_channels(cp) have zero weights and bias."""
    g = _gen("stem", b, S, cp, integer)
    if integer:
        img = torch.randint(-2, 3, (b, 3, S, S), generator=g).float()
        w4 = torch.randint(-1, 2, (cp, 3, 3, 3), generator=g).float()
        bias = torch.randint(-3, 4, (cp,), generator=g).float()
    else:
        img = torch.randn(b, 3, S, S, generator=g)
        w4 = torch.randn(cp, 3, 3, 3, generator=g) * 27 ** -0.5
        bias = torch.randn(cp, generator=g)
    w4[stem_zero_channels(cp)] = 0.0
    bias[stem_zero_channels(cp)] = 0.0
    return img, w4, bias, stem_ref(img, w4, bias)


def avgpool_ref(x, k):
    """fp64 k x k / stride k mean, NHWC in and out."""
    return F.avg_pool2d(x.double().permute(0, 3, 1, 2), k).permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def avgpool_case(b, H, C, k, coded=False):
    """(x [b,H,H,C], fp64 reference).  coded: x = its own flat NHWC index (exact in fp32 below 2^24; so are the window sums and the
    division by the power of two k^2): the pooled values name the elements that were read."""
    if coded:
        assert b * H * H * C * k * k < 2 ** 24 and k & (k - 1) == 0
        x = torch.arange(b * H * H * C, dtype=torch.float32).reshape(b, H, H, C)
    else:
        x = torch.randn(b, H, H, C, generator=_gen("pool", b, H, C, k))
    return x, avgpool_ref(x, k)


@functools.lru_cache(maxsize=None)
def tokens_case(b, HW, C):
    """(x [b,HW,C], pos [HW+1,C], fp32 x + pos[1:], fp64 mean(x) + pos[0])."""
    g = _gen("tokens", b, HW, C)
    x = torch.randn(b, HW, C, generator=g)
    pos = torch.randn(HW + 1, C, generator=g) * C ** -0.5
    return x, pos, x + pos[1:], x.double().mean(1) + pos[0].double()
