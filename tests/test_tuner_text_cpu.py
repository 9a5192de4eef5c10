"""The text format of fern_tuner_export / fern_tuner_import / FERN_GEMM_TILES, pinned line by line: what is accepted, what is refused,
what a line degrades to and the order of the export.  Import and export are pure host code: no device is ever initialised here.

The tuner's state is process-wide and cannot be cleared, so every line here carries an odd M that no other test and no benchmark shape
uses (4099, 5003, 6007, 7001, 7013, 7019) and the assertions look at those lines only."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from fashionern_aaai2024_amd import _lib
    return _lib.load()


def _export(lib):
    n = lib.fern_tuner_export(None, 0)
    import ctypes
    buf = ctypes.create_string_buffer(int(n) + 1)
    lib.fern_tuner_export(buf, int(n) + 1)
    text = buf.value.decode()
    assert text == "" or text.endswith("\n")
    return text.splitlines()


def _mine(lines, *ms):
    """The exported lines whose first M is one of `ms`, in export order."""
    return [ln for ln in lines if ln.split()[1] in {str(m) for m in ms}]


# every kind and every accepted form; (imported line, exported line)
CORPUS = [
    ("f32 4099 512 1024 0 0 8", "f32 4099 512 1024 0 0 8 0 8"),                          # single, short form
    ("f32 4099 512 1024 1 0 9 0 9", "f32 4099 512 1024 1 0 9 0 9"),                      # single, as exported
    ("f32 4099 768 1024 0 0 12 3840 11", "f32 4099 768 1024 0 0 12 3840 11"),            # bulk + remainder
    ("f32 4099 1024 1024 0 0 20 3840 4096", "f32 4099 1024 1024 0 0 20 3840 4096"),      # mixed, 256 x 128 macro-tiles
    ("f32 4099 1280 1024 0 0 21 3968 4099", "f32 4099 1280 1024 0 0 21 3968 4099"),      # mixed, 128 x 256: rows_a a multiple of 128 only
    ("f32 4099 512 2048 0 2000 8 0 8", "f32 4099 512 2048 0 2000 8 0 8"),                # split-K tag (1000 x ksplit) in the loader field
    ("f32x3 5003 512 1024 0 6", "f32x3 5003 512 1024 0 6 0 6"),                          # f32x3 single, short form: no loader field
    ("f32x3 5003 512 1024 2 7 0 7", "f32x3 5003 512 1024 2 7 0 7"),
    ("f32x3 5003 768 1024 0 20 4864 5003", "f32x3 5003 768 1024 0 20 4864 5003"),        # f32x3 mixed
    ("pair 5003 768 1024 0 3000 4099 512 1024 0 3000 1", "pair 5003 768 1024 0 3000 4099 512 1024 0 3000 1"),      # 3000: the f32x3 family's pairs
    ("pair 4099 1024 1024 0 0 5003 512 512 0 0 0", "pair 4099 1024 1024 0 0 5003 512 512 0 0 0"),
    ("bf16 4099 512 1024 0 1 7", "bf16 4099 512 1024 0 1 7"),
    ("bf16 4099 512 1024 0 0 9", "bf16 4099 512 1024 0 0 9"),                            # config 9: 64-element k tiles, K % 64 == 0
    ("fp8 4099 512 1024 0 2 5", "fp8 4099 512 1024 0 2 5"),
    ("mx8 4099 512 1024 0 4 11", "mx8 4099 512 1024 0 4 11"),
    ("mx8 4099 512 1024 1 13 10", "mx8 4099 512 1024 1 13 10"),                          # ob = bf16 output | block-scaled | output scales
    ("pairb 4099 768 1024 0 5 5003 512 512 0 1 0", "pairb 4099 768 1024 0 5 5003 512 512 0 1 0"),
    ("pairb 4099 768 1024 1 13 5003 512 512 1 1 1", "pairb 4099 768 1024 1 13 5003 512 512 1 1 1"),
    ("pairb 4099 768 3072 0 5 5003 512 2048 0 1 2", "pairb 4099 768 3072 0 5 5003 512 2048 0 1 2"),
]

# export order: f32x3 plans, f32 plans, pairs, the reduced-precision map (bf16 / fp8 / mx8 interleaved by key), pairb -- each in key order
# (M, N, K, epilogue, last key field)
EXPORT_ORDER = [
    "f32x3 5003 512 1024 0 6 0 6",
    "f32x3 5003 512 1024 2 7 0 7",
    "f32x3 5003 768 1024 0 20 4864 5003",
    "f32 4099 512 1024 0 0 8 0 8",
    "f32 4099 512 1024 1 0 9 0 9",
    "f32 4099 512 2048 0 2000 8 0 8",
    "f32 4099 768 1024 0 0 12 3840 11",
    "f32 4099 1024 1024 0 0 20 3840 4096",
    "f32 4099 1280 1024 0 0 21 3968 4099",
    "pair 4099 1024 1024 0 0 5003 512 512 0 0 0",
    "pair 5003 768 1024 0 3000 4099 512 1024 0 3000 1",
    "bf16 4099 512 1024 0 0 9",
    "bf16 4099 512 1024 0 1 7",
    "fp8 4099 512 1024 0 2 5",
    "mx8 4099 512 1024 0 4 11",
    "mx8 4099 512 1024 1 13 10",
    "pairb 4099 768 1024 0 5 5003 512 512 0 1 0",
    "pairb 4099 768 1024 1 13 5003 512 512 1 1 1",
    "pairb 4099 768 3072 0 5 5003 512 2048 0 1 2",
]

REFUSED = [
    # a configuration index out of range, in each family
    "f32 6007 512 1024 0 0 16", "f32 6007 512 1024 0 0 -1", "f32 6007 512 1024 0 0 4",      # 4: a retired slot of the table
    "f32 6007 512 1024 0 0 22 3840 4096",
    "f32x3 6007 512 1024 0 8", "f32x3 6007 512 1024 0 -1", "f32x3 6007 512 1024 0 22 3840 4096",
    "bf16 6007 512 1024 0 0 10", "bf16 6007 512 1024 0 0 -1", "fp8 6007 512 1024 0 2 6", "mx8 6007 512 1024 0 4 12",
    # K is not a multiple of the configuration's k tile (f32 0: 32, bf16 6: 64, fp8: 64, mx8: 128 whatever the configuration, mixed: 16)
    "f32 6007 512 1040 0 0 0", "bf16 6007 512 1056 0 0 6", "fp8 6007 512 1056 0 2 0", "mx8 6007 512 1088 0 4 8",
    "f32 6007 512 1032 0 0 20 3840 4096",
    # mixed plans: rows_a not a multiple of 256 (128 for 21), cfg_b below rows_a, cfg_b past M, a middle band that is no multiple of 128
    "f32 6007 640 1024 0 0 20 3968 4096", "f32 6007 640 1024 0 0 21 3904 6007", "f32 6007 640 1024 0 0 20 3840 3712",
    "f32 6007 640 1024 0 0 20 3840 6008", "f32 6007 640 1024 0 0 20 3840 3900", "f32 6007 640 1024 0 0 20 0 4096",
    "f32x3 6007 640 1024 0 20 3968 4096", "f32x3 6007 640 1024 0 21 3904 6007", "f32x3 6007 640 1024 0 20 3840 3712",
    "f32x3 6007 640 1024 0 20 3840",                                                   # a mixed f32x3 plan wants all three numbers
    # a line's kind against the `ob` bits of its key
    "bf16 6007 768 1024 0 5 0", "bf16 6007 768 1024 0 2 0", "fp8 6007 768 1024 0 0 0", "fp8 6007 768 1024 0 6 0", "mx8 6007 768 1024 0 2 0",
    "bf16 0 768 1024 0 0 0",
    # pair choices
    "pairb 6007 768 1024 0 5 5003 512 512 0 1 3", "pairb 6007 768 1024 0 5 5003 512 512 0 1 -1",
    # unknown kinds, truncated lines
    "int4 6007 512 1024 0 0 0", "F32 6007 512 1024 0 0 8", "6007 512 1024 0 0 8",
    "f32 6007 512 1024 0 0", "f32 6007 512 1024", "f32x3 6007 512 1024 0", "bf16 6007 512 1024 0 1", "mx8 6007",
    "pair 6007 768 1024 0 0 4099 512 1024 0 0", "pairb 6007 768 1024 0 5 5003 512 512 0 1", "f32 6007 512 1024 0 0 x",
]


def test_round_trip_keeps_every_accepted_form_and_the_export_order():
    lib = _lib()
    assert lib.fern_tuner_import("".join(src + "\n" for src, _ in CORPUS).encode()) == 0
    got = _mine(_export(lib), 4099, 5003)
    assert sorted(got) == sorted(want for _, want in CORPUS)
    assert got == EXPORT_ORDER
    # what was exported is accepted again and changes nothing
    assert lib.fern_tuner_import("".join(ln + "\n" for ln in got).encode()) == 0
    assert _mine(_export(lib), 4099, 5003) == EXPORT_ORDER


def test_refused_lines_leave_no_trace():
    lib = _lib()
    assert lib.fern_tuner_import(b"") == 0
    for line in REFUSED:
        assert lib.fern_tuner_import((line + "\n").encode()) == 0, line
    assert lib.fern_tuner_import("".join(ln + "\n" for ln in REFUSED).encode()) == 0
    assert lib.fern_tuner_import(b"\n\n") == 0
    assert lib.fern_tuner_import(b"f32 6007 512 1024 0 0") == 0      # truncated AND without its final newline
    assert _mine(_export(lib), 6007, 0) == []


def test_last_line_needs_no_newline():
    """The splitter takes the text's last line as it is: a COMPLETE line without a final newline is read like any other (only a line cut
    short is refused, above)."""
    lib = _lib()
    assert lib.fern_tuner_import(b"f32 7001 1536 1024 0 0 10 0 10\nbf16 7001 1536 1024 0 1 3") == 0
    assert _mine(_export(lib), 7001)[-1:] == ["bf16 7001 1536 1024 0 1 3"]
    assert "f32 7001 1536 1024 0 0 10 0 10" in _export(lib)


def test_bad_remainder_degrades_to_the_single_configuration():
    lib = _lib()
    text = ("f32 7001 512 1024 0 0 8 7001 11\n"       # rows_a >= M
            "f32 7001 512 1024 1 0 8 9000 11\n"
            "f32 7001 512 1024 2 0 8 3840 4\n"         # remainder configuration out of the table
            "f32 7001 512 1024 3 0 8 3840 16\n"
            "f32 7001 512 1040 0 0 8 3840 0\n"         # remainder's k tile (32) does not divide K
            "f32 7001 512 1024 4 0 8 -256 11\n"
            "f32 7001 512 1024 5 0 8 3840\n")          # no remainder configuration at all
    assert lib.fern_tuner_import(text.encode()) == 0
    got = [ln for ln in _mine(_export(lib), 7001) if ln.startswith("f32 7001 512 ")]
    assert got == ["f32 7001 512 1024 0 0 8 0 8", "f32 7001 512 1024 1 0 8 0 8", "f32 7001 512 1024 2 0 8 0 8", "f32 7001 512 1024 3 0 8 0 8",
                   "f32 7001 512 1024 4 0 8 0 8", "f32 7001 512 1024 5 0 8 0 8", "f32 7001 512 1040 0 0 8 0 8"]


def test_second_import_replaces_the_first():
    lib = _lib()
    first = ("f32 7013 512 1024 0 0 8\nf32x3 7013 512 1024 0 1\npair 7013 512 1024 0 0 7013 256 1024 0 0 1\nbf16 7013 512 1024 0 1 0\n"
             "fp8 7013 512 1024 0 2 0\nmx8 7013 512 1024 0 4 0\npairb 7013 512 1024 0 5 7013 256 1024 0 1 2\n")
    second = ("f32 7013 512 1024 0 0 12 3840 9\nf32x3 7013 512 1024 0 21 1280 7013\npair 7013 512 1024 0 0 7013 256 1024 0 0 0\n"
              "bf16 7013 512 1024 0 1 8\nfp8 7013 512 1024 0 2 3\nmx8 7013 512 1024 0 4 9\npairb 7013 512 1024 0 5 7013 256 1024 0 1 0\n")
    assert lib.fern_tuner_import(first.encode()) == 0
    assert len(_mine(_export(lib), 7013)) == 7
    assert lib.fern_tuner_import(second.encode()) == 0
    assert _mine(_export(lib), 7013) == ["f32x3 7013 512 1024 0 21 1280 7013", "f32 7013 512 1024 0 0 12 3840 9",
                                        "pair 7013 512 1024 0 0 7013 256 1024 0 0 0", "bf16 7013 512 1024 0 1 8", "fp8 7013 512 1024 0 2 3",
                                        "mx8 7013 512 1024 0 4 9", "pairb 7013 512 1024 0 5 7013 256 1024 0 1 0"]
    # a refused line for a stored key leaves the stored choice alone
    assert lib.fern_tuner_import(b"f32 7013 512 1024 0 0 16\nbf16 7013 512 1024 0 1 10\npairb 7013 512 1024 0 5 7013 256 1024 0 1 3\n") == 0
    assert len(_mine(_export(lib), 7013)) == 7 and "bf16 7013 512 1024 0 1 8" in _export(lib)


_CHILD = """
import ctypes
from fashionern_aaai2024_amd import _lib
lib = _lib.load()
assert lib.fern_tuner_import(b"") == 0
n = lib.fern_tuner_export(None, 0)
buf = ctypes.create_string_buffer(int(n) + 1)
lib.fern_tuner_export(buf, int(n) + 1)
print("EXPORT-BEGIN")
print(buf.value.decode(), end="")
print("EXPORT-END")
"""


def test_pin_file_is_read_once_for_every_kind(tmp_path):
    """FERN_GEMM_TILES is read once per process, so a fresh child: one line of each kind and one refused line in the file, exactly the
    accepted ones in the child's export (in export order).  The child imports nothing but the library and never opens a device."""
    accepted = ["f32x3 7019 512 1024 0 2 0 2", "f32 7019 512 1024 0 0 12 3840 11", "pair 7019 512 1024 0 0 7019 256 1024 0 0 1",
                "bf16 7019 512 1024 0 1 6", "fp8 7019 512 1024 0 3 4", "mx8 7019 512 1024 0 12 7", "pairb 7019 512 1024 0 5 7019 256 1024 0 1 2"]
    tiles = tmp_path / "tiles.txt"
    tiles.write_text("\n".join(["mx8 7019 512 1024 0 12 7", "pairb 7019 512 1024 0 5 7019 256 1024 0 1 2", "f32 7019 768 1024 0 0 16", "f32 7019 512 1024 0 0 12 3840 11",
                                "bf16 7019 512 1024 0 1 6", "pair 7019 512 1024 0 0 7019 256 1024 0 0 1", "fp8 7019 512 1024 0 3 4", "f32x3 7019 512 1024 0 2"]) + "\n")
    env = dict(os.environ, FERN_GEMM_TILES=str(tiles))
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    body = r.stdout.split("EXPORT-BEGIN\n", 1)[1].split("EXPORT-END", 1)[0]
    assert body.splitlines() == accepted
