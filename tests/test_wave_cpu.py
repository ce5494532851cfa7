"""The waveform front end without a GPU: the host tables (khg_frontend_tables) against the plain-Python
restatement on the bits and against recorded pins, frame counts and frame starts, the float32 host form against the float64
restatement within the derived bound, the bound's power to discriminate, edge values and the C symbols."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wave_cases as cases  # noqa: E402
import wave_ref as ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE_SHAPES = dict(cases.SHAPES, **{"22k1024": cases.SHAPE_1024})


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("high_freq", [0.0, -400.0])
@pytest.mark.parametrize("shape", sorted(TABLE_SHAPES))
def test_tables_equal_the_restatement_on_the_bits(shape, high_freq):
    import kaldi_hmm_gmm_amd as khg
    for win in cases.WINDOWS:
        o = ref.opts(window_type=win, high_freq=high_freq, **TABLE_SHAPES[shape])
        got, want = khg.frontend_tables(cases.lib_opts(o)), ref.tables_f32(o)
        L, S, N = ref.dims(o)
        assert (got["L"], got["S"], got["N"]) == (L, S, N)
        assert got["window"].shape == (L,) and got["twiddles"].shape == (N // 2, 2) and got["dct"].shape == (13, o["num_mel_bins"])
        for name in ("window", "mel_w", "dct", "lifter", "twiddles"):
            assert got[name].dtype == np.float32 and got[name].shape == want[name].shape, (win, name)
            assert (_bits(got[name]) == _bits(want[name])).all(), (win, name, int((_bits(got[name]) != _bits(want[name])).sum()))
        for name in ("mel_off", "mel_len"):
            assert got[name].dtype == np.int32 and (got[name] == want[name]).all(), (win, name)
        assert int(got["mel_len"].sum()) == len(got["mel_w"]) and (got["mel_off"] + got["mel_len"] <= N // 2).all()
        assert (got["mel_w"] > 0).all() and (got["mel_w"] <= 1).all()          # nonzero only strictly inside (left, right)
    if shape == "22k1024":
        assert (L, N) == (551, 1024)


def test_tables_recorded_pins():
    """bit patterns recorded once from the restatement (tests/golden/wave_pins.json): povey w[1], the first filter's run at the three
    shapes, dct[1][0]; and what a 2 pi / L window would give instead of 2 pi / (L - 1)"""
    import math

    import kaldi_hmm_gmm_amd as khg
    with open(os.path.join(HERE, "golden", "wave_pins.json")) as f:
        pins = json.load(f)
    for shape, kw in cases.SHAPES.items():
        t = khg.frontend_tables(cases.lib_opts(ref.opts(**kw)))
        pin = pins[shape]
        assert "%08x" % _bits(t["window"])[1] == pin["povey_w1"], shape
        assert [int(t["mel_off"][0]), int(t["mel_len"][0])] == pin["filter0"], shape
        assert "%08x" % _bits(t["dct"])[1, 0] == pin["dct10"], shape
        L = t["L"]
        wrong = np.float32(math.pow(0.5 - 0.5 * math.cos(2.0 * math.pi / L), 0.85))
        assert t["window"][1] != wrong and t["window"][0] == 0.0 and t["window"][L - 1] == t["window"][0]
        assert t["window"][1] == t["window"][L - 2]             # symmetric about (L - 1) / 2


@pytest.mark.parametrize("snip", [True, False])
def test_num_frames_and_frame_starts(snip):
    import kaldi_hmm_gmm_amd as khg
    o = ref.opts(snip_edges=snip)
    lo = cases.lib_opts(o)
    L, S = 400, 160
    assert ref.dims(o)[:2] == (L, S)
    want = {0: 0, 1: 0, L - 1: 0, L: 1, L + S - 1: 1, L + S: 2} if snip else {0: 0, 1: 0, L - 1: 2, L: 3, L + S - 1: 3, L + S: 4}
    for n, T in want.items():
        assert khg.num_frames(lo, n) == T == ref.num_frames(o, n), n
        st = khg.frame_starts(lo, n)
        assert st.tolist() == [ref.frame_start(o, t) for t in range(T)], n
        assert st.tolist() == [t * S + (0 if snip else S // 2 - L // 2) for t in range(T)]
    if not snip:
        assert khg.frame_starts(lo, L).tolist() == [-120, 40, 200]
        assert khg.num_frames(lo, S // 2) == 1 and khg.num_frames(lo, S // 2 - 1) == 0
    with pytest.raises(Exception):
        khg.num_frames(lo, -1)


@pytest.mark.parametrize("snip", [True, False])
def test_frame_offsets_are_the_prefix_sums_of_num_frames(snip):
    import kaldi_hmm_gmm_amd as khg
    for kw in cases.SHAPES.values():
        o = ref.opts(snip_edges=snip, **kw)
        lo = cases.lib_opts(o)
        lens = cases.batch_lengths(o)
        off = np.concatenate([[0], np.cumsum(lens)])
        fo = khg.frame_offsets(lo, off)
        assert fo.dtype == np.int64 and fo.tolist() == np.concatenate([[0], np.cumsum([ref.num_frames(o, n) for n in lens])]).tolist()
        assert np.diff(fo).tolist() == [khg.num_frames(lo, n) for n in lens]
    with pytest.raises(ValueError):
        khg.frame_offsets(lo, [0, 10, 5])
    with pytest.raises(Exception, match="dither"):
        khg.frame_offsets(khg.FrontendOptions(dither=1.0), [0, 10])


def test_reflection_is_repeated_until_inside():
    """n = 3 without snip_edges at a shift of 4 samples: one frame that starts at -198 and folds through the three samples again and
    again; the host form reads x[reflect(i)] exactly (a rectangular window without pre-emphasis or mean keeps the samples visible)"""
    import kaldi_hmm_gmm_amd as khg
    for n in (1, 2, 3, 7):
        for i in range(-40, 40):
            j = i % (2 * n)
            assert ref.reflect(i, n) == (2 * n - 1 - j if j >= n else j)
    assert [ref.reflect(i, 3) for i in range(-7, 0)] == [0, 0, 1, 2, 2, 1, 0] and [ref.reflect(i, 3) for i in range(3, 10)] == [2, 1, 0, 0, 1, 2, 2]
    o = ref.opts(kind="fbank", snip_edges=False, frame_shift_ms=0.25, window_type="rectangular", preemph_coeff=0.0, remove_dc_offset=False, use_energy=True)
    lo = cases.lib_opts(o)
    assert ref.dims(o)[1] == 4 and khg.num_frames(lo, 3) == 1 and khg.frame_starts(lo, 3).tolist() == [-198]
    x = np.array([1000.0, -2000.0, 3000.0], np.float32)
    got = khg.compute_fbank_feats(x, lo)
    want, det = ref.features(x, o, detail=True)
    assert got.shape == want.shape == (1, 24)
    assert det["frames"][0, :8].tolist() == [x[ref.reflect(-198 + i, 3)] for i in range(8)]
    # the raw energy is a sum of exact squares of whole numbers below 2^24 each: the float chains lose at most 400 roundings of the total
    assert abs(float(got[0, 0]) - want[0, 0]) <= 400 * 2.0 ** -24 + 2.0 ** -23 * abs(want[0, 0])
    bound = ref.log_mel_bound(o, det)
    assert (np.abs(got[:, 1:] - want[:, 1:]) <= bound).all()


def _host_vs_ref(shape, tone, kind, snip=True, n=None, seed=11):
    import kaldi_hmm_gmm_amd as khg
    kw = cases.SHAPES[shape]
    o = ref.opts(kind=kind, snip_edges=snip, **kw)
    L, S, _ = ref.dims(o)
    x = cases.noise(n or (L + 100 * S + 17), seed, tone=tone, samp_freq=kw["samp_freq"])
    lo = cases.lib_opts(o)
    got = khg.compute_mfcc_feats(x, lo) if kind == "mfcc" else khg.compute_fbank_feats(x, lo)
    want, det = ref.features(x, o, detail=True)
    lmb = ref.log_mel_bound(o, det)
    bound = ref.cepstra_bound(o, lmb) if kind == "mfcc" else lmb
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    return got, want, bound, lmb


@pytest.mark.parametrize("tone", [False, True])
@pytest.mark.parametrize("shape", sorted(cases.SHAPES))
def test_host_form_within_the_derived_bound(shape, tone):
    """float32 host form against the float64 restatement: every log-mel cell and every cepstrum within its own bound (K = 4 log2 N + 7
    is counted in DESIGN.md 7q, never fitted), and the bound itself at most 0.1 on these inputs, so that it means something.
    Measured (100 frames): largest error / bound 0.039 (log-mel) and 0.018 (cepstra); largest bound 0.031, at 8 kHz / 80 bins."""
    worst = {}
    for kind in ("fbank", "mfcc"):
        got, want, bound, lmb = _host_vs_ref(shape, tone, kind)
        ratio = np.abs(got - want) / bound
        worst[kind] = float(ratio.max())
        print("%s tone=%s %s: largest error %.3g, largest error / bound %.3g, largest log-mel bound %.3g" %
              (shape, tone, kind, float(np.abs(got - want).max()), worst[kind], float(lmb.max())))
        assert lmb.max() <= 0.1
        assert ratio.max() <= 1.0


def test_host_form_without_snip_edges_and_with_energies():
    import kaldi_hmm_gmm_amd as khg
    for raw in (True, False):
        o = ref.opts(kind="mfcc", snip_edges=False, use_energy=True, raw_energy=raw)
        x = cases.noise(3000, 4, tone=True)
        got = khg.compute_mfcc_feats(x, cases.lib_opts(o))
        want, det = ref.features(x, o, detail=True)
        assert got.shape == want.shape == (ref.num_frames(o, 3000), 13)
        bound = ref.cepstra_bound(o, ref.log_mel_bound(o, det))
        assert (np.abs(got[:, 1:] - want[:, 1:]) <= bound[:, 1:]).all()
        # the energy: a sum of L squares in float (at most L / 64 + 7 additions deep, one product each), five roundings before the square
        assert (np.abs(got[:, 0] - want[:, 0]) <= 40 * 2.0 ** -24 + 2.0 ** -23 * np.abs(want[:, 0])).all()


@pytest.mark.parametrize("variant,least", [("hamming", 0.5), ("no_preemph", 0.5), ("shift_filters", 0.5)])
def test_the_bound_discriminates(variant, least):
    """a wrong window, no pre-emphasis or filters off by one bin move some log-mel cell by at least 0.5, far outside every bound"""
    for shape, kw in cases.SHAPES.items():
        for tone in (False, True):
            o = ref.opts(kind="fbank", **kw)
            L, S, _ = ref.dims(o)
            x = cases.noise(L + 100 * S + 17, 11, tone=tone, samp_freq=kw["samp_freq"])
            want, det = ref.features(x, o, detail=True)
            moved = np.abs(ref.features(x, o, variant=variant) - want)
            print("%s %s tone=%s: largest move %.3g" % (variant, shape, tone, float(moved.max())))
            assert moved.max() >= least
            assert (moved > ref.log_mel_bound(o, det)).any()


def test_all_zero_utterance_is_finite():
    import kaldi_hmm_gmm_amd as khg
    x = np.zeros(2000, np.float32)
    fb = khg.compute_fbank_feats(x, khg.FrontendOptions(use_energy=1))
    floor = np.float32(np.log(np.float64(np.finfo(np.float32).eps)))
    assert fb.shape == (11, 24) and np.isfinite(fb).all() and (cases.ulps(fb, floor) <= 2).all()
    mf = khg.compute_mfcc_feats(x, None)
    assert mf.shape == (11, 13) and np.isfinite(mf).all()


def test_energy_floor_is_applied():
    import kaldi_hmm_gmm_amd as khg
    x = cases.noise(2000, 2) * np.float32(0.001)
    lo = khg.FrontendOptions(use_energy=1, energy_floor=0.0)
    free = khg.compute_mfcc_feats(x, lo)
    lo.energy_floor = 1e6
    floored = khg.compute_mfcc_feats(x, lo)
    assert (free[:, 0] < np.log(1e6)).all()
    assert (floored[:, 0] == np.float32(np.log(np.float64(np.float32(1e6))))).all() and (floored[:, 1:] == free[:, 1:]).all()
    lo.energy_floor = 1e-3                                      # below every frame's energy: nothing changes
    assert khg.compute_mfcc_feats(x, lo).tobytes() == free.tobytes()


def test_int16_equals_float():
    import kaldi_hmm_gmm_amd as khg
    x = cases.noise(3000, 8, tone=True)
    assert khg.compute_mfcc_feats(x.astype(np.int16), None).tobytes() == khg.compute_mfcc_feats(x, None).tobytes()
    lo = khg.FrontendOptions(samp_freq=8000.0, num_mel_bins=80, snip_edges=0)
    assert khg.compute_fbank_feats(x.astype(np.int16), lo).tobytes() == khg.compute_fbank_feats(x, lo).tobytes()


REFUSALS = [
    (dict(dither=1.0), "dither"), (dict(round_to_power_of_two=0), "round_to_power_of_two"), (dict(vtln_warp=1.1), "vtln_warp"),
    (dict(htk_compat=1), "htk_compat"), (dict(frame_length_ms=5.0), "padded window"), (dict(frame_length_ms=100.0), "padded window"),
    (dict(num_mel_bins=2), "num_mel_bins"), (dict(num_mel_bins=129), "num_mel_bins"), (dict(num_ceps=24), "num_ceps"),
]


@pytest.mark.parametrize("kw,word", REFUSALS)
def test_refusals_name_the_option(kw, word):
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _lib
    lo = khg.FrontendOptions(**kw)
    for call in (lambda: khg.num_frames(lo, 1000), lambda: khg.frontend_tables(lo), lambda: khg.frontend_dims(lo), lambda: khg.compute_mfcc_feats(np.zeros(1000), lo)):
        with pytest.raises(Exception, match=word):
            call()
    c = _lib.FrontendOptsC()
    _lib.lib.khg_frontend_opts_default(_lib.C.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    T = _lib.C.c_int64(-7)
    assert _lib.lib.khg_frontend_num_frames(_lib.C.byref(c), 1000, _lib.C.byref(T)) == -4 and T.value == -7       # KHG_E_UNSUPPORTED
    with pytest.raises(Exception):
        khg.FrontendOptions(no_such_option=1)


def test_options_defaults_agree():
    import kaldi_hmm_gmm_amd as khg
    from kaldi_hmm_gmm_amd import _lib
    c = _lib.FrontendOptsC()
    _lib.lib.khg_frontend_opts_default(_lib.C.byref(c))
    lo = khg.FrontendOptions()
    for name, _ in _lib.FrontendOptsC._fields_:
        assert getattr(lo, name) == getattr(c, name), name
    assert (lo.samp_freq, lo.frame_length_ms, lo.frame_shift_ms, lo.num_mel_bins, lo.num_ceps, lo.dither) == (16000.0, 25.0, 10.0, 23, 13, 0.0)
    assert khg.frontend_dims(lo) == {"L": 400, "S": 160, "N": 512, "num_mel_bins": 23, "num_ceps": 13, "dim": 13, "num_weights": int(khg.frontend_tables(lo)["mel_len"].sum())}


def test_symbols_exported_and_declared():
    from kaldi_hmm_gmm_amd import _lib
    root = os.path.dirname(HERE)
    so = os.path.join(root, "kaldi_hmm_gmm_amd", "libkhg_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    header = open(os.path.join(root, "include", "khg_hip.h")).read()
    for name in ("khg_frontend_opts_default", "khg_frontend_dims", "khg_frontend_num_frames", "khg_frontend_tables", "khg_frontend_create", "khg_frontend_destroy",
                 "khg_frontend_compute"):
        assert (" T " + name + "\n") in out and name in _lib.SIGNATURES and (" " + name + "(") in header, name
    # plain-C calls with NULLs are refused before anything is touched
    assert _lib.lib.khg_frontend_num_frames(None, 10, None) != 0
    assert _lib.lib.khg_frontend_dims(None, None) != 0
    assert _lib.lib.khg_frontend_tables(None, None, None, None, None, None, None, None) != 0
    assert _lib.lib.khg_frontend_create(None, None, None) != 0
    assert _lib.lib.khg_frontend_compute(None, None, 0, None, None, None, 0, None, None) != 0
    assert _lib.lib.khg_frontend_destroy(None) == 0


# ---- every option branch and FFT size (cases.OPTION_CASES) ----
CASES = list(cases.OPTION_CASES)


def test_option_case_constants_are_the_librarys():
    import kaldi_hmm_gmm_amd as khg
    assert (cases.TILE_FRAMES, cases.TILE_LDS_BYTES) == (khg.FE_TILE_FRAMES, khg.FEAT_TILE_LDS_BYTES)
    want = {"n1024": (551, 220, 1024), "n256_l160": (160, 80, 256), "l_eq_n_256": (256, 160, 256), "l_eq_n_512": (512, 160, 512),
            "shift_gt_len": (400, 480, 512), "shift_1": (400, 1, 512), "b128_8k": (200, 80, 256)}
    for name in CASES:
        o = cases.case_opts(name)
        d = khg.frontend_dims(cases.lib_opts(o))
        assert (d["L"], d["S"], d["N"]) == ref.dims(o) == want.get(name, (400, ref.dims(o)[1], 512)), name
        assert d["dim"] == cases.out_dim(o)


@pytest.mark.parametrize("name", CASES)
def test_option_case_tables_equal_the_restatement_on_the_bits(name):
    import kaldi_hmm_gmm_amd as khg
    o = cases.case_opts(name)
    got, want = khg.frontend_tables(cases.lib_opts(o)), ref.tables_f32(o)
    N, B, C = ref.dims(o)[2], o["num_mel_bins"], o["num_ceps"]
    assert got["dct"].shape == (C, B) and got["lifter"].shape == (C,)
    for tname in ("window", "mel_w", "dct", "lifter", "twiddles"):
        assert got[tname].dtype == np.float32 and got[tname].shape == want[tname].shape, tname
        assert (_bits(got[tname]) == _bits(want[tname])).all(), (tname, int((_bits(got[tname]) != _bits(want[tname])).sum()))
    for tname in ("mel_off", "mel_len"):
        assert got[tname].dtype == np.int32 and (got[tname] == want[tname]).all(), tname
    assert int(got["mel_len"].sum()) == len(got["mel_w"]) and (got["mel_off"] >= 0).all() and (got["mel_off"] + got["mel_len"] <= N // 2).all()
    assert (got["mel_w"] > 0).all() and (got["mel_w"] <= 1).all()      # every stored weight: an empty run stores none
    if name == "lifter0":
        assert (got["lifter"] == 1.0).all()
    if name in ("b128_16k", "b128_8k", "c128"):
        empty = [b for b, (_, ws) in enumerate(ref.mel_filters(o)) if not ws]
        assert len(empty) >= 1 and (got["mel_len"][empty] == 0).all()
        assert int((got["mel_len"] == 0).sum()) == len(empty) == {"b128_16k": 1, "b128_8k": 4, "c128": 1}[name]
    else:
        assert (got["mel_len"] > 0).all()


def _case_wave(name, o):
    L, S, N = ref.dims(o)
    n = L + (5 if N == 1024 else 20) * S + 17
    return cases.noise(n, 11, tone=True, samp_freq=o["samp_freq"], dc=cases.case_dc(name))


@pytest.mark.parametrize("name", CASES)
def test_option_case_host_form_within_the_derived_bound(name):
    """the float32 host form against the float64 restatement under every option set: every log-mel cell and every cepstrum within its
    own bound with K = ref.bound_roundings (counted in DESIGN.md 7q), the bound itself at most 0.1; for three cases also with the
    energy in column 0, raw and windowed, within the energy's bound of test_host_form_without_snip_edges_and_with_energies.
    Measured: largest error / bound 0.20 (FBANK at 128 bins), 0.059 at preemph0 (K = 57), 0.061 at nodc_rect_c0, below 0.014 elsewhere."""
    import kaldi_hmm_gmm_amd as khg
    variants = [dict()]
    if name in ("c1", "b128_16k", "nodc"):
        variants += [dict(use_energy=True, raw_energy=True), dict(use_energy=True, raw_energy=False)]
    for kw in variants:
        for kind in ("fbank", "mfcc"):
            o = cases.case_opts(name, kind=kind, **kw)
            x = _case_wave(name, o)
            lo = cases.lib_opts(o)
            got = khg.compute_mfcc_feats(x, lo) if kind == "mfcc" else khg.compute_fbank_feats(x, lo)
            want, det = ref.features(x, o, detail=True)
            assert got.dtype == np.float32 and got.shape == want.shape == (6 if name == "n1024" else ref.num_frames(o, len(x)), cases.out_dim(o))
            assert np.isfinite(got).all()
            lmb = ref.log_mel_bound(o, det)
            bound = ref.cepstra_bound(o, lmb) if kind == "mfcc" else lmb
            err = np.abs(got - want)
            if kw:
                assert (err[:, 0] <= 40 * 2.0 ** -24 + 2.0 ** -23 * np.abs(want[:, 0])).all()
                err, want = err[:, 1:], want[:, 1:]
                bound = bound[:, 1:] if kind == "mfcc" else bound
            if err.shape[1] == 0:                                    # c1 with use_energy: the energy alone
                assert (name, kind) == ("c1", "mfcc")
                continue
            ratio = err / bound
            print("%s %s %s: largest error %.3g, largest error / bound %.3g, largest log-mel bound %.3g (K = %d)" %
                  (name, kind, kw, float(err.max()), float(ratio.max()), float(lmb.max()), ref.bound_roundings(o)))
            assert lmb.max() <= 0.1
            assert (ratio <= 1.0).all()


@pytest.mark.parametrize("name", cases.KEEP_SHAPE + ["lifter0"])
def test_each_option_case_discriminates(name):
    """a condition on the inputs: the restatement under the case's options, on the case's own signal, differs from the restatement at
    the defaults beyond the case's own bound in at least half of the cells (some cell for nodc: under the povey window and c = 0.97 a
    constant offset reaches few bins) -- or a host form that ignored the option would agree with a kernel that ignores it"""
    kind = "mfcc" if name == "lifter0" else "fbank"
    o = cases.case_opts(name, kind=kind)
    base = ref.opts(kind=kind, num_ceps=o["num_ceps"])
    x = _case_wave(name, o)
    want, det = ref.features(x, o, detail=True)
    lmb = ref.log_mel_bound(o, det)
    bound = ref.cepstra_bound(o, lmb) if kind == "mfcc" else lmb
    moved = np.abs(ref.features(x, base) - want)
    if name == "lifter0":                                        # the lifter is 1 at c = 0 whatever Q is
        moved, bound = moved[:, 1:], bound[:, 1:]
    frac = float((moved > bound).mean())
    print("%s: largest move %.3g, largest move / bound %.3g, cells beyond the bound %.0f %%" % (name, float(moved.max()), float((moved / bound).max()), 100 * frac))
    assert (moved > bound).any()
    if name != "nodc":
        assert frac >= 0.5


def test_option_batch_lengths_hold_every_tile_shape():
    F = cases.TILE_FRAMES
    for name in CASES:
        for snip in (True, False):
            o = cases.case_opts(name, snip_edges=snip)
            lens = cases.option_batch_lengths(o)
            T = [ref.num_frames(o, n) for n in lens]
            assert T[:11] == [0, 1, 2, 3, 4, 5, F - 1, F, F + 1, 2 * F + 1, 37], (name, snip, T)
            assert len(lens) <= 13 and sum(T) <= 135 and max(T) == 37
            tiles = [min(F, t - a) for t in T for a in range(0, t, F)]
            assert {n % 4 for n in tiles} == {0, 1, 2, 3} and F in tiles
            if not snip:
                S = ref.dims(o)[1]
                assert lens[11:] == [n for n in (S // 2, S // 2 - 1) if n >= 0]


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("name", ["shift_gt_len", "shift_1", "n1024", "l_eq_n_256"])
def test_option_case_frame_offsets_and_starts(name, snip):
    """frame_offsets, num_frames and frame_starts against the restatement where S > L, S = 1, L is odd (551: S / 2 - L / 2 = 110 - 275
    truncates as C does) and L == N"""
    import kaldi_hmm_gmm_amd as khg
    o = cases.case_opts(name, snip_edges=snip)
    lo = cases.lib_opts(o)
    L, S, _ = ref.dims(o)
    lens = cases.option_batch_lengths(o)
    T = [ref.num_frames(o, n) for n in lens]
    fo = khg.frame_offsets(lo, np.concatenate([[0], np.cumsum(lens)]))
    assert fo.dtype == np.int64 and fo.tolist() == np.concatenate([[0], np.cumsum(T)]).tolist()
    for n, t in zip(lens, T):
        assert khg.num_frames(lo, n) == t
        st = khg.frame_starts(lo, n)
        assert st.dtype == np.int64 and st.tolist() == [ref.frame_start(o, i) for i in range(t)], n
    if name == "n1024" and not snip:
        assert khg.frame_starts(lo, lens[1]).tolist() == [110 - 275]
