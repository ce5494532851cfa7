"""Plain-Python restatement of DESIGN.md section 7q (compute-mfcc-feats, compute-fbank-feats) for the tests.  It shares no code with
the library: the tables are computed here in Python floats by the written operations (math.cos, math.pow, math.log, math.sin), the
transform is an explicit O(N^2) DFT in float64 and everything after it is float64.  Options are a plain dict (OPTS gives the
defaults); `variant` perturbs the rule on purpose for the tests that show the bounds discriminate."""
import math

import numpy as np

OPTS = dict(kind="mfcc", samp_freq=16000.0, frame_length_ms=25.0, frame_shift_ms=10.0, preemph_coeff=0.97, remove_dc_offset=True,
            window_type="povey", blackman_coeff=0.42, snip_edges=True, num_mel_bins=23, low_freq=20.0, high_freq=0.0, num_ceps=13,
            cepstral_lifter=22.0, use_energy=False, raw_energy=True, energy_floor=0.0, use_log_fbank=True, use_power=True)
FLT_EPS = 2.0 ** -23


def opts(**kw):
    o = dict(OPTS)
    for k in kw:
        assert k in o, k
    o.update(kw)
    return o


def f32(x):
    return float(np.float32(x))


def dims(o):
    sf = f32(o["samp_freq"])
    L = int(sf * 0.001 * f32(o["frame_length_ms"]))
    S = int(sf * 0.001 * f32(o["frame_shift_ms"]))
    N = 1
    while N < L:
        N *= 2
    return L, S, N


def num_frames(o, n):
    L, S, _ = dims(o)
    if o["snip_edges"]:
        return 0 if n < L else 1 + (n - L) // S
    return (n + S // 2) // S


def frame_start(o, t):
    L, S, _ = dims(o)
    return t * S if o["snip_edges"] else t * S + S // 2 - L // 2


def reflect(i, n):
    while i < 0 or i >= n:
        i = -i - 1 if i < 0 else 2 * n - 1 - i
    return i


def window(o):
    L = dims(o)[0]
    a = 2.0 * math.pi / (L - 1)
    kind, c = o["window_type"], f32(o["blackman_coeff"])
    w = []
    for i in range(L):
        x = float(i)
        if kind == "hanning":
            w.append(0.5 - 0.5 * math.cos(a * x))
        elif kind == "hamming":
            w.append(0.54 - 0.46 * math.cos(a * x))
        elif kind == "povey":
            w.append(math.pow(0.5 - 0.5 * math.cos(a * x), 0.85))
        elif kind == "rectangular":
            w.append(1.0)
        elif kind == "blackman":
            w.append(c - 0.5 * math.cos(a * x) + (0.5 - c) * math.cos(2.0 * a * x))
        else:
            raise ValueError(kind)
    return w


def mel(f):
    return 1127.0 * math.log(1.0 + f / 700.0)


def mel_filters(o):
    """-> per filter (first bin, [weights]) over the bins 0 .. N / 2 - 1; a weight is nonzero only strictly inside (left, right)"""
    _, _, N = dims(o)
    sf = f32(o["samp_freq"])
    B = o["num_mel_bins"]
    nyquist = 0.5 * sf
    high = f32(o["high_freq"])
    if high <= 0.0:
        high += nyquist
    width = sf / N
    lo, hi = mel(f32(o["low_freq"])), mel(high)
    delta = (hi - lo) / (B + 1)
    out = []
    for b in range(B):
        left, center, right = lo + b * delta, lo + (b + 1) * delta, lo + (b + 2) * delta
        first, ws = -1, []
        for k in range(N // 2):
            m = mel(width * k)
            if left < m < right:
                ws.append((m - left) / (center - left) if m <= center else (right - m) / (right - center))
                if first < 0:
                    first = k
        out.append((max(first, 0), ws))
    return out


def dct_matrix(o):
    B, C = o["num_mel_bins"], o["num_ceps"]
    n0, n1 = math.sqrt(1.0 / B), math.sqrt(2.0 / B)
    return [[n0 if c == 0 else n1 * math.cos(math.pi / B * (b + 0.5) * c) for b in range(B)] for c in range(C)]


def lifter(o):
    Q = f32(o["cepstral_lifter"])
    return [1.0 + 0.5 * Q * math.sin(math.pi * c / Q) if Q != 0.0 else 1.0 for c in range(o["num_ceps"])]


def twiddles(o):
    N = dims(o)[2]
    return [(math.cos(2.0 * math.pi * k / N), -math.sin(2.0 * math.pi * k / N)) for k in range(N // 2)]


def tables_f32(o):
    """the tables narrowed to float32 once, in the library's layout"""
    filt = mel_filters(o)
    return {
        "window": np.array(window(o), np.float64).astype(np.float32),
        "mel_off": np.array([f[0] for f in filt], np.int32),
        "mel_len": np.array([len(f[1]) for f in filt], np.int32),
        "mel_w": np.array([w for f in filt for w in f[1]], np.float64).astype(np.float32),
        "dct": np.array(dct_matrix(o), np.float64).astype(np.float32).reshape(o["num_ceps"], o["num_mel_bins"]),
        "lifter": np.array(lifter(o), np.float64).astype(np.float32),
        "twiddles": np.array(twiddles(o), np.float64).astype(np.float32),
    }


_DFT = {}


def dft_matrix(N):
    """rows k = 0 .. N / 2 - 1 of the DFT of N points, float64, phases reduced exactly (k n mod N) before the cosine"""
    if N not in _DFT:
        kn = (np.arange(N // 2)[:, None] * np.arange(N)[None, :]) % N
        ang = 2.0 * np.pi * kn / N
        _DFT[N] = (np.cos(ang), -np.sin(ang))
    return _DFT[N]


def features(wave, o, variant=None, detail=False):
    """float64 features of one utterance [T, dim].  variant: None, "hamming" (that window instead of the option's), "no_preemph",
    "shift_filters" (every filter one bin up).  detail: also the per-frame quantities the error bounds need."""
    L, S, N = dims(o)
    x = np.asarray(wave, np.float64)
    n = len(x)
    T = num_frames(o, n)
    B = o["num_mel_bins"]
    mfcc = o["kind"] == "mfcc"
    o2 = dict(o, window_type="hamming") if variant == "hamming" else o
    win = np.array(window(o2))
    c = 0.0 if variant == "no_preemph" else f32(o["preemph_coeff"])
    filt = mel_filters(o)
    if variant == "shift_filters":
        filt = [(min(off + 1, N // 2 - len(ws)), ws) for off, ws in filt]
    use_log = mfcc or o["use_log_fbank"]
    use_power = mfcc or o["use_power"]
    cr, ci = dft_matrix(N)
    frames = np.zeros((T, L))
    for t in range(T):
        s = frame_start(o, t)
        frames[t] = x[s:s + L] if (s >= 0 and s + L <= n) else [x[reflect(s + i, n)] for i in range(L)]
    mean = frames.mean(1) if o["remove_dc_offset"] else np.zeros(T)
    w = frames - mean[:, None]
    e_raw = (w * w).sum(1)
    pre = w.copy()
    if c != 0.0:
        pre[:, 1:] = w[:, 1:] - c * w[:, :-1]
        pre[:, 0] = w[:, 0] - c * w[:, 0]
    v = pre * win[None, :]
    e_win = (v * v).sum(1)
    pad = np.zeros((T, N))
    pad[:, :L] = v
    re, im = pad @ cr.T, pad @ ci.T
    mag = np.sqrt(re * re + im * im)
    spec = re * re + im * im if use_power else mag
    e = np.zeros((T, B))
    for b, (off, ws) in enumerate(filt):
        if ws:
            e[:, b] = spec[:, off:off + len(ws)] @ np.array(ws)
    lm = np.log(np.maximum(e, FLT_EPS)) if use_log else e
    energy = None
    if o["use_energy"]:
        energy = np.log(np.maximum(e_raw if o["raw_energy"] else e_win, FLT_EPS))
        if f32(o["energy_floor"]) > 0.0:
            energy = np.maximum(energy, math.log(f32(o["energy_floor"])))
    if mfcc:
        out = (lm @ np.array(dct_matrix(o)).T) * np.array(lifter(o))[None, :]
        if energy is not None:
            out[:, 0] = energy
    else:
        out = lm if energy is None else np.concatenate([energy[:, None], lm], axis=1)
    if detail:
        return out, {"frames": frames, "mean": mean, "win": win, "c": c, "mag": mag, "e": e, "filt": filt, "lm": lm}
    return out


def bound_roundings(o):
    """K of DESIGN.md 7q, the roundings (a relative 2^-24 each) on the longest path from a sample to a bin.  4 log2 N + 6 for the
    path itself: the mean's subtraction 1, pre-emphasis 2, the window 2, 4 for each of the log2 N - 1 stages, the post-pass 5.  The
    mean's own error -- ceil(L / 64) chain additions, 6 lane steps, inv_L's narrowing, one product -- enters every sample alike and
    pre-emphasis scales it by 1 - c: with c > 0 it is counted as 1 (0.26 of a rounding at c = 0.97; a c between 0 and 0.89 would
    need more and is not among the tests' cases), without remove_dc_offset there is no mean and the 1 is slack, and with c = 0 it
    keeps its full ceil(L / 64) + 8."""
    L, _, N = dims(o)
    K = 4 * int(round(math.log2(N))) + 6
    if o["remove_dc_offset"] and f32(o["preemph_coeff"]) == 0.0:
        return K + -(-L // 64) + 8
    return K + 1


def log_mel_bound(o, det):
    """|dX_k| <= delta = K 2^-24 sum_n (|x_n| + |mean|) (1 + c) win_n with K = bound_roundings(o) (4 log2 N + 7 at the
    defaults), and |d log e_b| <= [sum_k w_bk (2 |X_k| delta + delta^2)] / e_b + (len_b + 4) 2^-24 + 2^-23 max(1, |log e_b|).
    -> [T, B]"""
    K = bound_roundings(o)
    u = 2.0 ** -24
    delta = K * u * ((np.abs(det["frames"]) + np.abs(det["mean"])[:, None]) * (1.0 + det["c"]) * det["win"][None, :]).sum(1)      # [T]
    T, B = det["e"].shape
    bound = np.zeros((T, B))
    for b, (off, ws) in enumerate(det["filt"]):
        X = det["mag"][:, off:off + len(ws)]
        num = (np.array(ws)[None, :] * (2.0 * X * delta[:, None] + delta[:, None] ** 2)).sum(1)
        e = np.maximum(det["e"][:, b], FLT_EPS)
        bound[:, b] = num / e + (len(ws) + 4) * u + 2.0 ** -23 * np.maximum(1.0, np.abs(np.log(e)))
    return bound


def cepstra_bound(o, lm_bound):
    """sum_b |dct_cb| lifter_c times the log-mel bounds -> [T, C]"""
    D = np.abs(np.array(dct_matrix(o)))
    return (lm_bound @ D.T) * np.abs(np.array(lifter(o)))[None, :]
