#!/usr/bin/env python3
"""Times the waveform front end on one device: compute-mfcc-feats at 16 kHz / 23 bins / 13 cepstra and
compute-fbank-feats at 8 kHz / 80 bins, from float32 and from int16 samples resident in HBM.  About 30 M frames' worth of samples
go through in chunks that fit (the same chunk of whole-number noise each time: the kernel's time does not depend on the values); the
kernel is timed by the HIP events around it, and the whole synchronous call -- the host's frame counts and tile list, their upload,
the launch and the wait -- by the wall clock, through DeviceFrontend.compute and through compute_*_feats_batch on the same resident
handle.  In the same process a device-to-device copy that moves as many bytes as the call reads plus writes (the samples once, the
features once) is timed; the kernel is reported as a fraction of that copy's bandwidth.  Medians over the chunks.  Prints one JSON
line.

Usage: python tools/frontend_bench.py [--frames 30000000] [--chunk-utts 2000] [--utt-frames 500] [--reps 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import kaldi_hmm_gmm_amd as khg  # noqa: E402
from feat_bench import copy_ms, kernel_sums  # noqa: E402

CONFIGS = {
    "mfcc_16k_23_13": dict(kind=khg.FE_MFCC, samp_freq=16000.0, num_mel_bins=23, num_ceps=13),
    "fbank_8k_80": dict(kind=khg.FE_FBANK, samp_freq=8000.0, num_mel_bins=80),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30000000, help="frames in all, over the chunks")
    ap.add_argument("--chunk-utts", type=int, default=2000)
    ap.add_argument("--utt-frames", type=int, default=500, help="mean frames of an utterance (lengths vary by a quarter either way)")
    ap.add_argument("--reps", type=int, default=7, help="repetitions of the copy")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/frontend_bench.py needs a GPU: nothing is measured without one")
    ctx = khg.Context(0)
    device = "cuda:%d" % ctx.device
    rng = np.random.default_rng(20230420)
    out = {"command": "tools/frontend_bench.py " + " ".join(sys.argv[1:]), "results": {}}
    for name, kw in CONFIGS.items():
        lo = khg.FrontendOptions(**kw)
        d = khg.frontend_dims(lo)
        T = rng.integers(args.utt_frames * 3 // 4, args.utt_frames * 5 // 4 + 1, size=args.chunk_utts)
        lens = d["L"] + (T - 1) * d["S"] + rng.integers(0, d["S"], size=args.chunk_utts)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        frames = int(sum(khg.num_frames(lo, int(n)) for n in lens))
        chunks = max(1, -(-args.frames // frames))
        fe = khg.DeviceFrontend(ctx, lo)
        feats = torch.empty((frames, fe.dim), dtype=torch.float32, device=device)
        for stype, dt, code in (("float32", torch.float32, khg.WAVE_F32), ("int16", torch.int16, khg.WAVE_I16)):
            smp = torch.empty(int(off[-1]), dtype=torch.float32, device=device).normal_(0.0, 3000.0).round_().clamp_(-32768, 32767).to(dt)
            torch.cuda.synchronize()
            ms, wall, wall_py = [], [], []
            batch = khg.compute_mfcc_feats_batch if kw["kind"] == khg.FE_MFCC else khg.compute_fbank_feats_batch
            for c in range(chunks + 1):                       # the first chunk warms up
                ctx.sync()
                ctx.set_timing(True)
                fe.compute(off, None, smp.data_ptr(), code, feats.data_ptr())
                ctx.sync()
                k = kernel_sums(ctx)
                ctx.set_timing(False)
                t0 = time.perf_counter()                      # the same call without the events: synchronous, so the wall clock holds all of it
                fe.compute(off, None, smp.data_ptr(), code, feats.data_ptr())
                t1 = time.perf_counter()
                batch(ctx, (off, smp), fe, out=feats)
                t2 = time.perf_counter()
                if c > 0:
                    ms.append(k["k_fe_wave"])
                    wall.append(1e3 * (t1 - t0))
                    wall_py.append(1e3 * (t2 - t1))
            moved = int(off[-1]) * smp.element_size() + 4 * frames * fe.dim
            cp = copy_ms(torch, moved, device, args.reps)
            med = float(np.median(ms))
            out["results"][name + "_" + stype] = {
                "frames_per_chunk": frames, "chunks": chunks, "frames": frames * chunks, "samples_per_chunk": int(off[-1]), "dim": fe.dim,
                "kernel_ms_per_chunk": round(med, 4), "call_wall_ms_per_chunk": round(float(np.median(wall)), 4),
                "batch_call_wall_ms_per_chunk": round(float(np.median(wall_py)), 4), "utts_per_chunk": args.chunk_utts, "kernel_ms_total": round(float(np.sum(ms)), 3), "frames_per_s": round(frames / (1e-3 * med), 0),
                "bytes_read_plus_written_per_chunk": moved, "gb_per_s": round(moved / (1e6 * med), 1),
                "copy_ms_same_bytes": round(cp, 4), "copy_gb_per_s": round(moved / (1e6 * cp), 1), "fraction_of_copy_bandwidth": round(cp / med, 4),
            }
            del smp
        fe.close()
        del feats
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
