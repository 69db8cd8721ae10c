"""include/fs2hip_postnet.h on the host: its one entry point is exported and bound in a table of
its own, the ctypes mirror of its descriptor has the C layout, the build id covers the header, the
argument checks answer without a GPU, and the runtime switch reads as documented."""
import ctypes
import os
import subprocess
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fs2hip_postnet.h")


def test_postnet_header_symbols_exported_and_bound():
    from fs2amd import _lib

    declared = _lib.header_symbols(HEADER)
    assert declared == sorted(_lib.SIGNATURES_POSTNET) == ["fs2_pn_head3"], declared
    assert not set(declared) & set(_lib.header_symbols(_lib.HEADER))
    assert "fs2hip_postnet.h" in _lib.EXTRA_HEADERS and _lib.HEADER_POSTNET == HEADER
    lib = _lib.load()
    fn = lib.fs2_pn_head3
    res, args = _lib.SIGNATURES_POSTNET["fs2_pn_head3"]
    assert fn.restype is res and list(fn.argtypes) == list(args)


def test_pn_head3_desc_layout_matches_header():
    from fs2amd import _lib

    cls = _lib.PnHead3Desc
    names = [f[0] for f in cls._fields_]
    src = "#include <stdio.h>\n#include <stddef.h>\n#include \"fs2hip_postnet.h\"\nint main(void){" + "".join(
        f'printf("{n} %zu\\n", offsetof(fs2_pn_head3_desc, {n}));' for n in names) + \
        'printf("size %zu\\n", sizeof(fs2_pn_head3_desc)); }\n'
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "t.c"), "w") as f:
        f.write(src)
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")],
                   check=True)
    out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split()
    got = dict(zip(out[::2], map(int, out[1::2])))
    assert got.pop("size") == ctypes.sizeof(cls)
    assert got == {n: getattr(cls, n).offset for n in names}


def test_pn_head3_rejects_bad_arguments_without_a_gpu():
    from fs2amd import _lib

    lib = _lib.load()
    assert lib.fs2_pn_head3(None, None) == _lib.FS2_EINVAL
    d = _lib.PnHead3Desc()  # all-null descriptor
    assert lib.fs2_pn_head3(ctypes.byref(d), None) == _lib.FS2_EINVAL
    d.x, d.mel_w, d.mel_b, d.mel, d.out = 256, 512, 768, 1024, 2048
    for i in range(3):
        d.w[i], d.bias[i] = 4096, 8192
    d.B, d.T, d.x_rows, d.x_row_stride, d.mel_row_stride, d.out_row_stride = 2, 8, 16, 256, 80, 512
    d.x_row_stride = 128  # rows narrower than the decoder's 256 channels
    assert lib.fs2_pn_head3(ctypes.byref(d), None) == _lib.FS2_EINVAL
    d.x_row_stride, d.x_rows = 256, 15  # no row map: one decoder row per padded row
    assert lib.fs2_pn_head3(ctypes.byref(d), None) == _lib.FS2_EINVAL
    d.x_rows, d.w[2] = 16, None
    assert lib.fs2_pn_head3(ctypes.byref(d), None) == _lib.FS2_EINVAL
    d.w[2], d.B = 4096, 0  # an empty batch launches nothing
    assert lib.fs2_pn_head3(ctypes.byref(d), None) == _lib.FS2_OK


def test_switch_reads_like_pn_head(monkeypatch):
    from fs2amd import runtime as R

    monkeypatch.delenv("FS2_PN_HEAD3", raising=False)
    assert R.pn_head3_on()
    monkeypatch.setenv("FS2_PN_HEAD3", "0")
    assert not R.pn_head3_on()
    monkeypatch.setenv("FS2_PN_HEAD3", "1")
    assert R.pn_head3_on()
