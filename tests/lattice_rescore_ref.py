"""Plain Python / numpy restatement of gmm-rescore-lattice and lattice-boost-ali on the dict of arrays that
DeviceLattices.download() gives (tests/lattice_ops_ref.FIELDS plus "start"): the yardstick of tests/test_lattice_rescore_cpu.py (the
host Lattice) and tests/test_gpu_lattice_rescore.py (the device).

The rules.  Every arc with ilabel != 0 leaves a state of some frame t (an emitting arc goes from frame t to frame t + 1):
  rescore   acoustic_cost := -(acoustic_scale * ll(t, id2pdf[ilabel])), one float32 multiply and a sign
  boost     graph_cost := fl(graph_cost + fl(-b * e)), e = 0 where tid2phone[ilabel] == tid2phone[ali[t]], max_silence_error where they
            differ and the arc's phone is a silence phone, 1 otherwise
Epsilon arcs and everything else are copied."""
import numpy as np

F = np.float32
SUCCEEDED, NO_PATH, NO_REF = 1, 8, 512


def arc_frames(lat):
    """the frame of every arc's source state"""
    n = np.diff(np.asarray(lat["arc_begin"], np.int64))
    return np.repeat(np.asarray(lat["frame"], np.int32), n)


def _copy(lat):
    return {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in lat.items()}


def rescore_from_ll(lat, ll, scale):
    """ll: callable (frame, transition-id) -> float32 score.  -> the rescored lattice"""
    out = _copy(lat)
    fr = arc_frames(lat)
    s = F(scale)
    for a, (t, il) in enumerate(zip(fr, lat["ilabel"])):
        if il != 0:
            out["acoustic_cost"][a] = F(-(s * F(ll(int(t), int(il)))))
    return out


def rescore_exact(lat, exact, bound, id2pdf, scale):
    """exact / bound: [num_pdfs][T] float64 from helpers.exact_loglikes (every pdf, this utterance's features).
    -> (float64 cost per arc, NaN on epsilon arcs; the bound B of every arc's cell, 0 on epsilon arcs)"""
    fr = arc_frames(lat)
    cost = np.full(len(fr), np.nan)
    B = np.zeros(len(fr))
    for a, (t, il) in enumerate(zip(fr, lat["ilabel"])):
        if il != 0:
            p = int(id2pdf[il])
            cost[a] = -(float(F(scale)) * exact[p, t])
            B[a] = bound[p, t]
    return cost, B


def boost(lat, tid2phone, silence_phones, ali, b, max_silence_error):
    out = _copy(lat)
    fr = arc_frames(lat)
    nb, mse = F(-F(b)), F(max_silence_error)
    sil = set(int(x) for x in silence_phones)
    for a, (t, il) in enumerate(zip(fr, lat["ilabel"])):
        if il == 0:
            continue
        ph, ref = int(tid2phone[il]), int(tid2phone[ali[t]])
        e = F(0.0) if ph == ref else (mse if ph in sil else F(1.0))
        out["graph_cost"][a] = F(lat["graph_cost"][a] + F(nb * e))
    return out


def boost_status(lat, num_tids, ali):
    """the KHG_LAT_* bits khg_lattices_boost gives this utterance"""
    if len(lat["frame"]) == 0:
        return NO_PATH
    T = int(lat["frame"][-1])
    if len(ali) == 0 or len(ali) != T or any(x < 1 or x > num_tids for x in ali):
        return NO_REF
    return SUCCEEDED


def empty():
    z, f = np.zeros(0, np.int32), np.zeros(0, np.float32)
    return {"frame": z, "graph_state": z, "tot_cost": f, "extra_cost": f, "final_cost": f, "arc_begin": np.zeros(1, np.int32),
            "ilabel": z, "olabel": z, "graph_cost": f, "acoustic_cost": f, "nextstate": z, "start": -1}


def cell_keys(lats, id2pdf, frame_off):
    """(pdf << 32) | feature row of every emitting arc of a batch of lattices (the keys khg_lattices_rescore sorts)"""
    keys = []
    for u, lat in enumerate(lats):
        fr = arc_frames(lat)
        for t, il in zip(fr, lat["ilabel"]):
            if il != 0:
                keys.append((int(id2pdf[il]) << 32) | (int(frame_off[u]) + int(t)))
    return np.asarray(keys, np.int64)
