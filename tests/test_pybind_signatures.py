"""The package's Python surface against the reference's pybind11 surface ("same Python names, kwargs").

tests/golden/pybind_signatures.json is an interface schema extracted by tools/extract_ref_signatures.py from the
in-scope /root/reference/kaldi-hmm-gmm/python/csrc/*.cc (class / member / function names, py::arg names in order,
which of them have defaults).  Every entry must be callable on `kaldi_hmm_gmm_amd` with the reference's keyword
names; names outside SURVEY §8 are waived explicitly in the fixture (`out_of_scope_names`), nothing else is.
"""
import inspect
import json
import os
import re

import pytest

import kaldi_hmm_gmm_amd as khg

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "pybind_signatures.json")) as f:
    SCHEMA = json.load(f)
WAIVED = SCHEMA["out_of_scope_names"]


def _split_top(s):
    parts, d, cur = [], 0, ""
    for c in s:
        if c in "([{":
            d += 1
        elif c in ")]}":
            d -= 1
        if c == "," and d == 0:
            parts.append(cur.strip()); cur = ""
        else:
            cur += c
    if cur.strip():
        parts.append(cur.strip())
    return parts


def overloads(obj, name):
    """[(argnames, has_default)] for every overload of a pybind11 function (from its docstring) or the one signature
    of a Python function; `self` dropped."""
    if inspect.isfunction(obj) or inspect.ismethod(obj) or (inspect.isclass(obj) and not _is_pybind(obj)):
        sig = inspect.signature(obj)
        ps = [p for p in sig.parameters.values() if p.name != "self" and p.kind not in (p.VAR_POSITIONAL, p.VAR_KEYWORD)]
        return [([p.name for p in ps], [p.default is not p.empty for p in ps])]
    doc = obj.__doc__ or ""
    out = []
    for line in doc.splitlines():
        m = re.match(r"^\s*(?:\d+\.\s+)?%s\((.*)\)\s*(?:->.*)?$" % re.escape(name), line)
        if not m or m.group(1).startswith("*args"):
            continue
        names, defs = [], []
        for a in _split_top(m.group(1)):
            if a in ("/", "*"):
                continue
            nm = a.split(":")[0].split("=")[0].strip()
            if nm == "self":
                continue
            names.append(nm)
            defs.append(re.search(r"[^=!<>]=[^=]", a.split(":", 1)[1] if ":" in a else a) is not None)
        out.append((names, defs))
    return out


def _is_pybind(cls):
    return type(cls).__name__ == "pybind11_type"


def _members():
    for cname, c in sorted(SCHEMA["classes"].items()):
        if cname in WAIVED:
            continue
        for i, m in enumerate(c["members"]):
            if "%s.%s" % (cname, m["name"]) in WAIVED:
                continue
            yield pytest.param(cname, m, id="%s.%s#%d" % (cname, m["name"], i))


def test_fixture_covers_every_binding_file_in_scope():
    assert len(SCHEMA["classes"]) >= 20 and len(SCHEMA["functions"]) >= 12
    assert set(SCHEMA["in_scope_files"]).isdisjoint(SCHEMA["out_of_scope_files"])
    # waivers are names only from the agreed out-of-scope list (lattice decoders, H transducer, k-means clustering)
    assert all(re.search(r"out of scope|needs ", why) for why in WAIVED.values())


@pytest.mark.parametrize("cname", sorted(c for c in SCHEMA["classes"] if c not in WAIVED))
def test_class_present_with_reference_bases(cname):
    cls = getattr(khg, cname)
    assert inspect.isclass(cls)
    for b in SCHEMA["classes"][cname]["bases"]:
        if b.startswith("Py"):        # pybind trampoline, not a Python-visible base
            continue
        assert issubclass(cls, getattr(khg, b)), "%s must derive from %s" % (cname, b)


@pytest.mark.parametrize("cname,m", list(_members()))
def test_member_matches_reference(cname, m):
    cls = getattr(khg, cname)
    name, kind = m["name"], m["kind"]
    where = "%s:%d" % (SCHEMA["classes"][cname]["file"], m["line"])
    if name == "__pickle__":
        assert hasattr(cls, "__getstate__") and hasattr(cls, "__setstate__") or not _is_pybind(cls), where
        return
    if kind in ("def_property", "def_property_readonly", "def_readwrite", "def_readonly"):
        if hasattr(cls, name):
            attr = inspect.getattr_static(cls, name)
            assert not inspect.isroutine(attr) or isinstance(attr, property), "%s.%s must be a property (%s)" % (cname, name, where)
            if kind in ("def_readwrite", "def_property") and isinstance(attr, property):
                assert attr.fset is not None, "%s.%s must be writable (%s)" % (cname, name, where)
        else:       # a plain Python class may keep it as an instance attribute set in __init__
            assert not _is_pybind(cls), "%s.%s missing (%s)" % (cname, name, where)
            assert name in inspect.signature(cls).parameters or name in getattr(cls, "__annotations__", {}) \
                or name in inspect.getsource(cls), "%s.%s missing (%s)" % (cname, name, where)
        return
    assert hasattr(cls, name), "%s.%s missing (%s)" % (cname, name, where)
    want = [a["name"] for a in m["args"]]
    want_def = [a["has_default"] for a in m["args"]]
    if name == "__init__":
        ovl = overloads(cls if not _is_pybind(cls) else cls.__init__, cls.__name__ if not _is_pybind(cls) else "__init__")
    else:
        ovl = overloads(getattr(cls, name), name)
    if want:
        ok = [(n, d) for n, d in ovl if n[:len(want)] == want and all(d[len(want):])]
        assert ok, "%s.%s: no overload takes the reference's (%s) -- have %s (%s)" % (cname, name, ", ".join(want), [n for n, _ in ovl], where)
        if name == "__init__" and not _is_pybind(cls):
            # a Python class folds the reference's overloads into one signature with defaults: only require that the
            # reference's defaulted arguments are defaulted here too
            assert any(all(dd or not wd for dd, wd in zip(d, want_def)) for _, d in ok), where
        else:
            assert any(d[:len(want)] == want_def for _, d in ok), \
                "%s.%s: defaults differ from the reference's %s (%s)" % (cname, name, list(zip(want, want_def)), where)
    elif m.get("lambda_arity") is not None and ovl:
        assert any(len(n) - sum(d) <= m["lambda_arity"] <= len(n) for n, d in ovl), \
            "%s.%s: reference takes %d positional arguments, have %s (%s)" % (cname, name, m["lambda_arity"], ovl, where)


@pytest.mark.parametrize("f", [pytest.param(f, id=f["name"]) for f in SCHEMA["functions"] if f["name"] not in WAIVED])
def test_function_matches_reference(f):
    fn = getattr(khg, f["name"])
    want = [a["name"] for a in f["args"]]
    want_def = [a["has_default"] for a in f["args"]]
    ovl = overloads(fn, f["name"])
    where = "%s:%d" % (f["file"], f["line"])
    if want:
        ok = [(n, d) for n, d in ovl if n[:len(want)] == want and all(d[len(want):])]
        assert ok, "%s: no overload takes (%s) -- have %s (%s)" % (f["name"], ", ".join(want), [n for n, _ in ovl], where)
        # pybind lets a defaulted argument precede required ones (add_transition_probs.disambig_syms); a Python def
        # cannot, so only the reference's REQUIRED arguments must stay required
        assert any(all(wd or not dd for dd, wd in zip(d, want_def)) for _, d in ok), where
    elif f.get("lambda_arity") is not None and ovl:
        assert any(len(n) - sum(d) <= f["lambda_arity"] <= len(n) for n, d in ovl), where


def test_enum_values_exported():
    for ename, e in SCHEMA["enums"].items():
        cls = getattr(khg, ename)
        for v in e["values"]:
            assert hasattr(cls, v), "%s.%s" % (ename, v)
            if e["export_values"]:
                assert getattr(khg, v) == getattr(cls, v), "%s must be exported at module level" % v


@pytest.mark.parametrize("f", [pytest.param(f, id=f["name"]) for f in SCHEMA["scripts"]])
def test_script_function_matches_reference(f):
    """scripts/gmm_*.py: same argument names in the same order, the same arguments defaulted to the same values;
    anything this package adds (verbose=, randn=) comes after them and is defaulted."""
    fn = getattr(khg, f["name"])
    ps = list(inspect.signature(fn).parameters.values())
    want = f["args"]
    assert [p.name for p in ps[:len(want)]] == [a["name"] for a in want], "%s (%s:%d)" % (f["name"], f["file"], f["line"])
    for p, a in zip(ps, want):
        assert (p.default is not p.empty) == a["has_default"], "%s.%s" % (f["name"], a["name"])
        if a["has_default"]:
            assert repr(p.default) == a["default"] or p.default == eval(a["default"]), "%s.%s default %r vs %s" % (f["name"], a["name"], p.default, a["default"])
    assert all(p.default is not p.empty for p in ps[len(want):])


@pytest.mark.parametrize("name", ["k1_last", "k3_last", "k2_tail", "k3_planes"])
def test_device_set_reports_what_ran(name):
    """the library's own getters on UtteranceSet (no counterpart in the reference): bound, no argument besides the set"""
    ovl = overloads(getattr(khg.UtteranceSet, name), name)
    assert ovl == [([], [])], ovl
