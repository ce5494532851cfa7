"""Options of the default K1's launch shape (KHG_OPT_K1_LAUNCH, _K1_PGRID, _K1_PROF): declared in the header, named in the Python
binding, validated by the library -- through khg_ctx_set_option's check and through the environment seeding -- without a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KHG_E_ARG = -1


def _header():
    with open(os.path.join(ROOT, "include", "khg_hip.h")) as f:
        return f.read()


def _opt(name):
    return int(re.search(r"#define %s (\d+)" % name, _header()).group(1))


def test_header_declares_the_options_and_the_error_code():
    h = _header()
    assert re.search(r"#define KHG_E_ARG \(%d\)" % KHG_E_ARG, h)
    ids = [_opt(n) for n in ("KHG_OPT_K1_LAUNCH", "KHG_OPT_K1_PGRID", "KHG_OPT_K1_PROF")]
    assert len(set(ids)) == 3 and max(ids) < _opt("KHG_OPT_COUNT")
    for env in ("KHG_K1_LAUNCH=auto|chunk|persistent", "KHG_K1_PGRID", "KHG_K1_PROF"):
        assert env in h


def test_python_binding_names_every_option():
    with open(os.path.join(ROOT, "kaldi_hmm_gmm_amd", "csrc", "khg_pybind.cpp")) as f:
        src = f.read()
    names = re.search(r"names\[KHG_OPT_COUNT\] = \{(.*?)\};", src, re.S).group(1)
    names = re.findall(r'"(\w+)"', names)
    assert len(names) == _opt("KHG_OPT_COUNT")
    assert names[_opt("KHG_OPT_K1_LAUNCH")] == "k1_launch" and names[_opt("KHG_OPT_K1_PGRID")] == "k1_pgrid"
    assert names[_opt("KHG_OPT_K1_PROF")] == "k1_prof"


def test_launch_option_values_through_set_option_check():
    from kaldi_hmm_gmm_amd import _lib

    launch = _opt("KHG_OPT_K1_LAUNCH")
    for v in (0, 1, 2):
        assert _lib.lib.khg_option_check(launch, v) == 0
    for v in (-1, 3, 4, 100, -(2**31), 2**31 - 1):
        assert _lib.lib.khg_option_check(launch, v) == KHG_E_ARG
        assert b"0 .. 2" in _lib.lib.khg_last_error()
    pgrid = _opt("KHG_OPT_K1_PGRID")
    assert _lib.lib.khg_option_check(pgrid, 0) == 0 and _lib.lib.khg_option_check(pgrid, 2) == 0
    assert _lib.lib.khg_option_check(pgrid, -1) == KHG_E_ARG
    assert _lib.lib.khg_option_check(_opt("KHG_OPT_COUNT"), 0) == KHG_E_ARG and _lib.lib.khg_option_check(-1, 0) == KHG_E_ARG
    # every option's default-like value 0 or its documented range start still passes (the table has one row per option)
    assert _lib.lib.khg_option_check(_opt("KHG_OPT_K1_FORM"), 1) == KHG_E_ARG        # the removed form keeps its refusal


@pytest.mark.parametrize("text,want", [("0", 0), ("1", 1), ("2", 2), ("auto", 0), ("chunk", 1), ("persistent", 2)])
def test_launch_option_through_the_environment(text, want):
    from kaldi_hmm_gmm_amd import _lib

    opt, val = C.c_int(-1), C.c_int(-1)
    assert _lib.lib.khg_option_from_env(b"KHG_K1_LAUNCH", text.encode(), C.byref(opt), C.byref(val)) == 0
    assert opt.value == _opt("KHG_OPT_K1_LAUNCH") and val.value == want


@pytest.mark.parametrize("text", ["3", "-1", "17", "resident", "Persistent", "2x"])
def test_launch_option_refused_through_the_environment(text):
    from kaldi_hmm_gmm_amd import _lib

    opt, val = C.c_int(-1), C.c_int(-1)
    rc = _lib.lib.khg_option_from_env(b"KHG_K1_LAUNCH", text.encode(), C.byref(opt), C.byref(val))
    if text == "2x":
        assert rc == 0 and val.value == 2          # atoi's reading of a number with a tail, as for every other variable
    else:
        assert rc == KHG_E_ARG and opt.value == -1 and val.value == -1


def test_environment_table_keeps_the_older_variables():
    from kaldi_hmm_gmm_amd import _lib

    opt, val = C.c_int(-1), C.c_int(-1)
    assert _lib.lib.khg_option_from_env(b"KHG_K1_ORDER", b"xcd", C.byref(opt), C.byref(val)) == 0
    assert (opt.value, val.value) == (_opt("KHG_OPT_K1_ORDER"), 4)
    assert _lib.lib.khg_option_from_env(b"KHG_K3_VALU", b"1", C.byref(opt), C.byref(val)) == 0
    assert (opt.value, val.value) == (_opt("KHG_OPT_K3_FORM"), 2)
    assert _lib.lib.khg_option_from_env(b"KHG_K1_PGRID", b"2", C.byref(opt), C.byref(val)) == 0 and val.value == 2
    assert _lib.lib.khg_option_from_env(b"KHG_NO_SUCH", b"1", C.byref(opt), C.byref(val)) == KHG_E_ARG
