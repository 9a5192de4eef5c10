"""Dump and compare: the shared half of the tests/_*_dump.py scripts, and the comparer of what they save.

A dump script states a `compute(eng)` that returns {name: array} (or one array) from seeded inputs, and hands it to `main`: one engine
for the run, closed at the end, the result saved to the path that is the command line's last argument.  `raw` is the form of a result
that may be large: its bytes, or their digest.

A change that is meant to move no bit is checked by running a dump script on both builds and comparing the two files:

    python tests/_dump.py diff a.npz b.npz

prints the number of arrays, the names present on one side only and the names whose bytes (or shape, or dtype) differ, and exits
non-zero if there is any such name.  A script, not a collected test; `diff` needs numpy only."""
import hashlib
import sys

import numpy as np

RAW_LIMIT = 65536


def raw(t):
    """uint8 array of a tensor's bytes; an array above 64 KiB as its SHA-256 digest (32 bytes)."""
    import torch
    b = t.detach().cpu().contiguous().view(torch.uint8).numpy().reshape(-1)
    return b.copy() if b.size <= RAW_LIMIT else np.frombuffer(hashlib.sha256(b.tobytes()).digest(), dtype=np.uint8).copy()


def main(compute, path=None):
    """Run `compute` on an engine of its own and save what it returns to `path` (default: the last command-line argument): a dict with
    np.savez, a single array with np.save."""
    import torch
    from fashionern_aaai2024_amd.engine import FernEngine
    path = path or sys.argv[-1]
    eng = FernEngine("cuda:0")
    try:
        out = compute(eng)
        torch.cuda.synchronize()
    finally:
        eng.close()
    if isinstance(out, dict):
        np.savez(path, **out)
        print(f"{len(out)} arrays -> {path}")
    else:
        np.save(path, out)
        print(f"1 array -> {path}")


def _load(path):
    z = np.load(path)
    return {"": z} if isinstance(z, np.ndarray) else {k: z[k] for k in z.files}


def diff(path_a, path_b, out=sys.stdout):
    """Print the comparison of two dumps; the number of names that are missing on a side or differ."""
    a, b = _load(path_a), _load(path_b)
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = [k for k in sorted(set(a) & set(b))
              if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
    print(f"{len(a)} arrays in {path_a}, {len(b)} in {path_b}, {len(set(a) & set(b)) - len(differ)} equal bit for bit", file=out)
    for title, names in ((f"only in {path_a}", only_a), (f"only in {path_b}", only_b), ("differ", differ)):
        print(f"{title}: {len(names)}" + "".join(f"\n  {k}" for k in names), file=out)
    return len(only_a) + len(only_b) + len(differ)


if __name__ == "__main__":
    if len(sys.argv) != 4 or sys.argv[1] != "diff":
        sys.exit("usage: python tests/_dump.py diff a.npz b.npz")
    sys.exit(1 if diff(sys.argv[2], sys.argv[3]) else 0)
