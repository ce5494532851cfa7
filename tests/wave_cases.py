"""Shared inputs of the waveform front end's tests: the shapes, the option translation between the restatement's
dict and the library's FrontendOptions, the test signals and an ulp measure."""
import numpy as np

import wave_ref as ref

# the three shapes of the issue: 16 kHz / 23 bins / 13 cepstra, 16 kHz / 40 bins, 8 kHz / 80 bins (the reference recipe's filterbank)
SHAPES = {
    "16k23": dict(samp_freq=16000.0, num_mel_bins=23, num_ceps=13),
    "16k40": dict(samp_freq=16000.0, num_mel_bins=40, num_ceps=13),
    "8k80": dict(samp_freq=8000.0, num_mel_bins=80, num_ceps=13),
}
SHAPE_1024 = dict(samp_freq=22050.0, num_mel_bins=40, num_ceps=13)     # L = 551, N = 1024
WINDOWS = ["povey", "hamming", "hanning", "rectangular", "blackman"]


TILE_FRAMES = 16                  # khg.FE_TILE_FRAMES and khg.FEAT_TILE_LDS_BYTES: the tests assert that these are the library's
TILE_LDS_BYTES = 64 * 1024
LDS_CEILING = "lds_ceiling"       # a frame_shift_ms that case_opts replaces by the largest shift whose tile fits TILE_LDS_BYTES

# name -> overrides on ref.opts() (16 kHz / 23 bins / 13 cepstra unless stated), each named for the kernel line it reaches
OPTION_CASES = {
    "win_hamming": dict(window_type="hamming"),                             # the table staging at another window
    "win_hanning": dict(window_type="hanning"),
    "win_rectangular": dict(window_type="rectangular"),
    "win_blackman": dict(window_type="blackman"),
    "blackman_c03": dict(window_type="blackman", blackman_coeff=0.3),
    "preemph0": dict(preemph_coeff=0.0),                                     # `c != 0` false
    "preemph1": dict(preemph_coeff=1.0),                                     # the upper end of the accepted range
    "nodc": dict(remove_dc_offset=False),                                    # mean = 0
    "nodc_rect_c0": dict(window_type="rectangular", preemph_coeff=0.0, remove_dc_offset=False),      # samples reach the FFT untouched
    "n1024": dict(SHAPE_1024),                                               # logM = 9, four butterfly trips a lane, LDS above 48 KiB
    "n256_l160": dict(frame_length_ms=10.0, frame_shift_ms=5.0),             # L = 160, N = 256
    "l_eq_n_256": dict(frame_length_ms=16.0),                                # L == N: `i < L` is never false
    "l_eq_n_512": dict(frame_length_ms=32.0),
    "shift_gt_len": dict(frame_shift_ms=30.0),                               # S > L: gaps inside the staged span
    "shift_1": dict(frame_shift_ms=0.0625),                                  # S = 1: a span of 15 + L
    "band": dict(low_freq=300.0, high_freq=-400.0),                          # other filter runs
    "b128_16k": dict(num_mel_bins=128),                                      # two filters a lane, an empty filter
    "b128_8k": dict(samp_freq=8000.0, num_mel_bins=128),
    "b3": dict(num_mel_bins=3, num_ceps=3),                                  # three lanes busy
    "b65": dict(num_mel_bins=65, num_ceps=65),                               # lane 0 alone takes a second filter and a second cepstrum
    "c128": dict(num_mel_bins=128, num_ceps=128),                            # the DCT loop's second trip
    "c1": dict(num_ceps=1),                                                  # one cepstrum; with use_energy the energy alone
    "lifter0": dict(cepstral_lifter=0.0, num_ceps=23),                       # C == B, a lifter of ones
    "lds_ceiling": dict(frame_shift_ms=LDS_CEILING),                         # the last launch the LDS limit accepts
}
KEEP_SHAPE = [k for k, v in OPTION_CASES.items() if not ({"samp_freq", "frame_length_ms", "frame_shift_ms", "num_mel_bins", "num_ceps"} & set(v))]


def lds_bytes(L, S, N, n_w, B, dim):
    """the dynamic LDS of one tile"""
    return 4 * ((TILE_FRAMES - 1) * S + 2 * L + N + n_w + 3 * B + 4 * (3 * N // 2 + 128) + TILE_FRAMES * dim)


def out_dim(o):
    return o["num_ceps"] if o["kind"] == "mfcc" else o["num_mel_bins"] + (1 if o["use_energy"] else 0)


def lds_ceiling_shift(o):
    """the largest S whose tile fits TILE_LDS_BYTES at o's other options, from the restatement's filters"""
    o = dict(o, frame_shift_ms=1.0)                              # neither L, N nor the filters depend on the shift
    L, _, N = ref.dims(o)
    n_w = sum(len(ws) for _, ws in ref.mel_filters(o))
    rest = lds_bytes(L, 0, N, n_w, o["num_mel_bins"], out_dim(o))
    return (TILE_LDS_BYTES - rest) // (4 * (TILE_FRAMES - 1))


def case_opts(name, **kw):
    """the restatement's options of a case; kw on top of the case's overrides (kind, snip_edges, use_energy ..)"""
    o = ref.opts(**dict(OPTION_CASES[name], **kw))
    if o["frame_shift_ms"] == LDS_CEILING:
        S = lds_ceiling_shift(o)
        o["frame_shift_ms"] = S * 1000.0 / o["samp_freq"]        # S / 16 at 16 kHz: exact in float32
        assert ref.dims(o)[1] == S
    return o


def option_batch_lengths(o, seed=7):
    """eleven utterances of 0, 1, 2, 3, 4, 5, F - 1, F, F + 1, 2 F + 1 and 37 frames under o's own edge mode (F the kernel's tile): every
    tile shape, every residue of a tile's frames mod 4 (every pattern of idle waves), 133 frames in all; each the shortest length
    of that many frames plus a few samples.  Without snip_edges also S / 2 samples and S / 2 - 1: one frame and none."""
    L, S, _ = ref.dims(o)
    F = TILE_FRAMES
    rng = np.random.default_rng(seed)
    counts = [0, 1, 2, 3, 4, 5, F - 1, F, F + 1, 2 * F + 1, 37]
    extra = [int(rng.integers(0, S)) for _ in counts]
    if o["snip_edges"]:
        return [max(L - 1 - e, 0) if T == 0 else L + (T - 1) * S + e for T, e in zip(counts, extra)]
    lens = [0 if T == 0 else T * S - S // 2 + e for T, e in zip(counts, extra)]          # T = (n + S / 2) / S
    return lens + [n for n in (S // 2, S // 2 - 1) if n >= 0]


def option_waves(o, dc=0.0, seed=200):
    """the batch of option_batch_lengths: cases.noise, every third utterance with the tone, `dc` added before rounding and clipping"""
    return [noise(n, seed + i, tone=(i % 3 == 0), samp_freq=o["samp_freq"], dc=dc) for i, n in enumerate(option_batch_lengths(o))]


def case_dc(name):
    """+2000 on every sample for the cases without DC removal: a mean that is kept moves every cell"""
    return 2000.0 if name.startswith("nodc") else 0.0


def lib_opts(o):
    """the restatement's dict -> FrontendOptions"""
    import kaldi_hmm_gmm_amd as khg
    win = {"povey": khg.WIN_POVEY, "hamming": khg.WIN_HAMMING, "hanning": khg.WIN_HANNING, "rectangular": khg.WIN_RECTANGULAR, "blackman": khg.WIN_BLACKMAN}
    kw = {k: (int(v) if isinstance(v, bool) else v) for k, v in o.items() if k not in ("kind", "window_type")}
    return khg.FrontendOptions(kind=khg.FE_MFCC if o["kind"] == "mfcc" else khg.FE_FBANK, window_type=win[o["window_type"]], **kw)


def noise(n, seed, tone=False, samp_freq=16000.0, dc=0.0):
    """rounded Gaussian noise (sigma 3000), with or without an 8000-amplitude 440 Hz tone, `dc` added before rounding and clipping:
    float32 holding whole numbers"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 3000.0
    if tone:
        x = x + 8000.0 * np.sin(2.0 * np.pi * 440.0 * np.arange(n) / samp_freq)
    return np.clip(np.round(x + dc), -32768, 32767).astype(np.float32)


def ulps(got, want):
    """|got - want| in units of float32 ulp(want)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


def batch_lengths(o, seed=5):
    """about 40 utterance lengths: 0, 1, 3, L - 1, L, L + S - 1, L + S, the lengths that give F - 1, F and F + 1 frames for the kernel's
    tile of F frames (and 2 F, 2 F + 1), a spread of short ones and a few of 300 to 700 frames"""
    import kaldi_hmm_gmm_amd as khg
    L, S, _ = ref.dims(o)
    F = khg.FE_TILE_FRAMES
    rng = np.random.default_rng(seed)

    def with_frames(T):                                        # the shortest utterance of T frames under snip_edges, plus a few samples
        return L + (T - 1) * S + int(rng.integers(0, S))

    lens = [0, 1, 3, L - 1, L, L + S - 1, L + S] + [with_frames(T) for T in (F - 1, F, F + 1, 2 * F, 2 * F + 1)]
    lens += [with_frames(int(T)) for T in rng.integers(2, 60, size=24)]
    lens += [with_frames(int(T)) for T in (300, 457, 700)]
    lens += [0, S // 2, S // 2 - 1]                            # without snip_edges: the shortest utterance with a frame, and one below it
    return lens
