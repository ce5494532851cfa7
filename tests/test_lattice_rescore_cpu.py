"""gmm-rescore-lattice and lattice-boost-ali on the host: Lattice.rescore / Lattice.boost against the plain
restatement (tests/lattice_rescore_ref.py) on the bits, the refusals that need no device, and the new C-ABI symbols.  No GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_ops_ref as ops  # noqa: E402
import lattice_post_cases as cases  # noqa: E402
import lattice_rescore_ref as rr  # noqa: E402
from test_lattice_ops_cpu import _hand, _lattice, _same_lattice  # noqa: E402

F = np.float32
INF = np.inf


def _all_lattices():
    c = dict(cases.hand_built())
    c.update(cases.geometry())
    c["one_path"] = cases.one_path()
    c["dead_states"] = cases.dead_states()[0]
    c.update(hand_made())
    return c


def hand_made():
    c = {}
    # an epsilon arc between two emitting ones
    c["eps_between"] = _hand([(0, INF), (1, INF), (1, INF), (2, 0.0)],
                             [(0, 3, 0, 0.5, 1.0, 1), (1, 0, 7, 0.25, 0.125, 2), (2, 4, 0, 0.75, 2.0, 3)])
    # two arcs of different states sharing the cell (frame 1, id 5), and two parallel arcs with one id
    c["shared_cell"] = _hand([(0, INF), (1, INF), (1, INF), (2, 0.0), (2, 1.0)],
                             [(0, 1, 0, 0.5, 1.0, 1), (0, 2, 0, 0.1, 3.0, 2), (1, 5, 0, 0.2, 1.5, 3), (2, 5, 0, 0.3, 2.5, 4), (2, 5, 0, 0.4, 0.5, 3)])
    # a silence / a non-silence / the matching phone on one frame (ids 1-2: phone 1 = silence, 3-4: phone 2, 5-6: phone 3)
    c["three_phones"] = _hand([(0, INF), (1, INF), (1, INF), (1, INF), (2, 0.0)],
                              [(0, 1, 0, 0.5, 1.0, 1), (0, 3, 0, 0.25, 2.0, 2), (0, 5, 0, 0.125, 3.0, 3), (1, 2, 0, 0.0, 1.0, 4), (2, 6, 0, 0.0, 1.0, 4),
                               (3, 4, 0, -0.0, 1.0, 4)])
    return c


def _table(lat, seed, n=None):
    """random scores [num_tids + 1][T] for a lattice"""
    T = int(lat["frame"][-1]) if len(lat["frame"]) else 0
    n = int(lat["ilabel"].max()) + 1 if n is None and len(lat["ilabel"]) else (n or 1)
    return np.random.default_rng(seed).normal(scale=30.0, size=(n, max(T, 1))).astype(F)


@pytest.mark.parametrize("scale", [1.0, 0.1, -2.5])
def test_rescore_equals_the_restatement_on_the_bits(scale):
    n_em = n_eps = 0
    for k, (name, lat) in enumerate(sorted(_all_lattices().items())):
        tab = _table(lat, k)
        want = rr.rescore_from_ll(lat, lambda t, il: tab[il, t], scale)
        L = _lattice(lat)
        _same_lattice(L.rescore(tab, acoustic_scale=scale), want, (name, "array"))
        _same_lattice(L.rescore(lambda t, il: float(tab[il, t]), scale), want, (name, "callable"))
        _same_lattice(L, lat, (name, "the input is untouched"))
        em = lat["ilabel"] != 0
        assert ops.bits(want["acoustic_cost"][~em]) == ops.bits(lat["acoustic_cost"][~em]), name       # epsilon arcs keep theirs
        n_em += int(em.sum()); n_eps += int((~em).sum())
    assert n_em > 500 and n_eps > 50


def test_rescore_with_zero_scores_zeroes_exactly_the_emitting_arcs():
    for name, lat in sorted(_all_lattices().items()):
        tab = np.zeros_like(_table(lat, 0))
        for scale in (1.0, 0.1, 7.0):
            got = _lattice(lat).rescore(tab, scale)
            em = lat["ilabel"] != 0
            ac = np.asarray(got.acoustic_cost)
            assert (ac[em] == 0.0).all(), name
            assert ops.bits(ac[~em]) == ops.bits(lat["acoustic_cost"][~em]), name
            for k in ops.FIELDS:
                if k != "acoustic_cost":
                    assert np.asarray(getattr(got, k)).tobytes() == lat[k].tobytes(), (name, k)


def test_rescore_shared_cell_gets_equal_bits_and_empty_stays_empty():
    lat = hand_made()["shared_cell"]
    tab = _table(lat, 3)
    got = np.asarray(_lattice(lat).rescore(tab).acoustic_cost)
    assert got[2] == got[3] == got[4] == -tab[5, 1]
    e = rr.empty()
    _same_lattice(_lattice(e).rescore(np.zeros((3, 1), F)), e, "empty")
    _same_lattice(_lattice(e).boost([0, 1, 1], [1], [], 0.5, 0.0), e, "empty boost")


TID2PHONE = np.array([0, 1, 1, 2, 2, 3, 3], np.int32)


@pytest.mark.parametrize("mse", [0.0, 0.5])
def test_boost_three_phones_on_one_frame(mse):
    lat = hand_made()["three_phones"]
    b = 0.3
    ali = [3, 6]             # phone 2 on frame 0, phone 3 on frame 1
    got = _lattice(lat).boost(TID2PHONE, [1], ali, b, mse)
    want = rr.boost(lat, TID2PHONE, [1], ali, b, mse)
    _same_lattice(got, want, mse)
    g = np.asarray(got.graph_cost)
    nb = F(-F(b))
    # frame 0: silence arc (id 1), matching arc (id 3), other arc (id 5)
    assert g[0] == F(F(0.5) + F(nb * F(mse))) and g[1] == F(0.25) and g[2] == F(F(0.125) + nb)
    # frame 1: silence (id 2), matching phone 3 (id 6), phone 2 (id 4, graph cost -0.0)
    assert g[3] == F(F(0.0) + F(nb * F(mse))) and ops.bits(g[4:5]) == ops.bits([F(0.0) + F(nb * F(0.0))]) and g[5] == F(F(-0.0) + nb)
    for k in ops.FIELDS:
        if k != "graph_cost":
            assert np.asarray(getattr(got, k)).tobytes() == lat[k].tobytes(), k


def test_boost_equals_the_restatement_and_b_zero_is_the_identity():
    n = 0
    for k, (name, lat) in enumerate(sorted(_all_lattices().items())):
        rng = np.random.default_rng(100 + k)
        nt = max(int(lat["ilabel"].max()), 2)
        t2p = np.concatenate([[0], rng.integers(1, 5, nt)]).astype(np.int32)
        sil = [int(t2p[1])]
        T = int(lat["frame"][-1])
        ali = rng.integers(1, nt + 1, T).astype(np.int32)
        for b, mse in ((0.1, 0.0), (1.75, 0.5), (-0.5, 2.0)):
            _same_lattice(_lattice(lat).boost(t2p, sil, ali, b, mse), rr.boost(lat, t2p, sil, ali, b, mse), (name, b, mse))
        _same_lattice(_lattice(lat).boost(t2p, sil, ali, 0.0, 0.5), lat, (name, "b = 0"))
        assert rr.boost_status(lat, nt, ali) == rr.SUCCEEDED
        n += 1
    assert n >= 20
    # boosting and rescoring commute: they touch different arrays
    lat = cases.hand_built()["epsilon_skips"]
    tab = _table(lat, 9)
    t2p = np.concatenate([[0], 1 + np.arange(int(lat["ilabel"].max())) % 3]).astype(np.int32)
    ali = [1, 2]
    a = _lattice(lat).boost(t2p, [1], ali, 0.4, 0.0).rescore(tab, 1.0)
    b = _lattice(lat).rescore(tab, 1.0).boost(t2p, [1], ali, 0.4, 0.0)
    _same_lattice(a, {**{k: np.asarray(getattr(b, k)) for k in ops.FIELDS}, "start": b.start}, "commute")


def test_host_refusals():
    lat = hand_made()["three_phones"]
    L = _lattice(lat)
    with pytest.raises(RuntimeError, match="finite"):
        L.rescore(np.zeros((7, 2), F), float("inf"))
    with pytest.raises(RuntimeError, match="outside loglikes"):
        L.rescore(np.zeros((3, 2), F))               # id 6 is not in the table
    with pytest.raises(RuntimeError, match="finite"):
        L.boost(TID2PHONE, [1], [3, 6], float("nan"), 0.0)
    with pytest.raises(RuntimeError, match="finite"):
        L.boost(TID2PHONE, [1], [3, 6], 0.1, float("inf"))
    with pytest.raises(RuntimeError, match="silence phone 9"):
        L.boost(TID2PHONE, [1, 9], [3, 6], 0.1, 0.0)
    with pytest.raises(RuntimeError, match="frames"):
        L.boost(TID2PHONE, [1], [3], 0.1, 0.0)       # a short alignment
    with pytest.raises(RuntimeError, match="outside 1"):
        L.boost(TID2PHONE, [1], [3, 0], 0.1, 0.0)
    with pytest.raises(RuntimeError, match="ilabel"):
        L.boost(TID2PHONE[:5], [1], [3, 4], 0.1, 0.0)     # the lattice carries ids 5 and 6
    assert rr.boost_status(lat, 6, [3]) == rr.NO_REF and rr.boost_status(lat, 6, [3, 0]) == rr.NO_REF
    assert rr.boost_status(lat, 6, []) == rr.NO_REF and rr.boost_status(rr.empty(), 6, []) == rr.NO_PATH


def test_c_abi_symbols_and_null_arguments():
    from kaldi_hmm_gmm_amd import _lib
    for name in ("khg_lattices_rescore", "khg_lattices_boost", "khg_lattices_op_status"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    out = C.c_void_p()
    st = _lib.RescoreStatsC()
    assert _lib.lib.khg_lattices_rescore(None, None, None, None, None, 1.0, 0, C.byref(st), C.byref(out)) == -1      # KHG_E_ARG
    assert b"khg_lattices_rescore" in _lib.lib.khg_last_error()
    assert _lib.lib.khg_lattices_boost(None, None, 0, None, 0, None, None, None, None, 0.1, 0.0, None, C.byref(out)) == -1
    assert _lib.lib.khg_lattices_op_status(None, None) == -1
    assert C.sizeof(_lib.RescoreStatsC) == 24


def test_transition_id_to_phone_array():
    from kaldi_hmm_gmm_amd import synth
    m = synth.make_model(6, 2, 5, seed=3)
    _, tm = synth.host_objects(m)
    a = tm.transition_id_to_phone_array()
    assert len(a) == tm.num_transition_ids + 1 and a[0] == 0
    assert a[1:] == [tm.transition_id_to_phone(i) for i in range(1, tm.num_transition_ids + 1)]
    assert len(a) == len(tm.transition_id_to_pdf_array())
