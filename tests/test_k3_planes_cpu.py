"""K3's split feature records without a device: the getter (khg_utts_k3_planes) is declared, exported, bound and refuses bad arguments;
the option (KHG_OPT_K3_PLANES) is in the header, the Python names and the environment table.  What the records hold and that both
fills of the LDS image give the same statistics: tests/test_gpu_k3_planes.py."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KHG_E_ARG = -1


def _header():
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as fh:
        return fh.read()


def test_k3_planes_entry_point():
    name = "khg_utts_k3_planes"
    from kaldi_hmm_gmm_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "kaldi_hmm_gmm_amd", "libkhg_hip.so")], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bint %s\(" % name, _header()) and name in _lib.SIGNATURES and re.search(r" T %s$" % name, out, re.M)
    import kaldi_hmm_gmm_amd as khg
    assert hasattr(khg.UtteranceSet, "k3_planes")


def test_k3_planes_getter_refuses_bad_arguments():
    from kaldi_hmm_gmm_amd import _lib
    b, p, u = C.c_int64(7), C.c_int64(7), C.c_int32(7)
    assert _lib.lib.khg_utts_k3_planes(None, C.byref(b), C.byref(p), C.byref(u)) == KHG_E_ARG
    assert b"khg_utts_k3_planes" in _lib.lib.khg_last_error()
    assert (b.value, p.value, u.value) == (7, 7, 7)
    assert _lib.lib.khg_utts_k3_planes(None, None, None, None) == KHG_E_ARG


def test_option_is_declared_named_and_seeded():
    h = _header()
    opt = int(re.search(r"#define KHG_OPT_K3_PLANES (\d+)", h).group(1))
    assert opt < int(re.search(r"#define KHG_OPT_COUNT (\d+)", h).group(1)) and "KHG_K3_PLANES=auto|off|on" in h
    with open(os.path.join(ROOT, "kaldi_hmm_gmm_amd", "csrc", "khg_pybind.cpp")) as fh:
        names = re.findall(r'"(\w+)"', re.search(r"names\[KHG_OPT_COUNT\] = \{(.*?)\};", fh.read(), re.S).group(1))
    assert names[opt] == "k3_planes"
    from kaldi_hmm_gmm_amd import _lib
    assert all(_lib.lib.khg_option_check(opt, v) == 0 for v in (0, 1, 2))
    assert _lib.lib.khg_option_check(opt, 3) == KHG_E_ARG and _lib.lib.khg_option_check(opt, -1) == KHG_E_ARG
    for text, want in (("auto", 0), ("off", 1), ("on", 2), ("0", 0), ("2", 2)):
        o, v = C.c_int(-1), C.c_int(-1)
        assert _lib.lib.khg_option_from_env(b"KHG_K3_PLANES", text.encode(), C.byref(o), C.byref(v)) == 0
        assert (o.value, v.value) == (opt, want)
    o, v = C.c_int(-1), C.c_int(-1)
    assert _lib.lib.khg_option_from_env(b"KHG_K3_PLANES", b"maybe", C.byref(o), C.byref(v)) == KHG_E_ARG
