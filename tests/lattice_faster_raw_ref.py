"""The raw lattice of the lattice-faster decoder, restated in plain Python on tests/lattice_faster_ref.py (the yardstick of
tests/test_lattice_faster_raw_cpu.py and tests/test_gpu_lattice_faster_raw.py).

LatticeFasterDecoder::GetRawLattice (reference csrc/lattice-faster-decoder.cc:101-192) as this project's order-faithful decoder
implies it -- the FST that lattice_faster_ref.LatticeFasterDecoder.get_best_path enumerates:

  states   one per token that survives FinalizeDecoding, numbered by frame, then in TopSortTokens order inside the frame with the gaps
           removed; frame, graph_state (the graph state the token was created for), tot_cost (as stored, cost offsets included),
           extra_cost (after the final pruning)
  arcs     per state, one per surviving forward link in the link list's order (head first); ilabel, olabel, graph_cost,
           acoustic_cost = fl(link.acoustic_cost - cost_offsets[frame]) for an emitting link and 0 for an epsilon link, nextstate
  finals   last frame: final_costs_[tok] (+inf without an entry) when any final state was reached, else 0 on every token
  start    state 0
  empty    whenever DecodeUtteranceLatticeFaster does not succeed

The graph state of a token: the restatement creates tokens in three places (InitDecoding, FindOrAddToken, and ProcessNonemitting's
own copy of FindOrAddToken), each right after the HashList lookup of the state, and keeps every token of a frame in the HashList
until the list is cleared.  So the subclass below records (token, key) of every Elem whenever the list is cleared -- which covers
all three places without copying any of them.

The lattice comes back as the dict of arrays of tests/lattice_ops_ref.py.  numpy only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_faster_ref as ref  # noqa: E402
import lattice_ops_ref as ops  # noqa: E402

F = np.float32
INF = F(np.inf)


class _RecordingHashList(ref.HashList):
    def __init__(self, sink):
        super().__init__()
        self.sink = sink

    def clear(self):
        for key, tok in self.items():
            if tok is not None:
                self.sink[tok.uid] = key
        return super().clear()


class RawLatticeFasterDecoder(ref.LatticeFasterDecoder):
    """lattice_faster_ref.LatticeFasterDecoder that also knows the graph state of every token (graph_state_of[uid])."""

    def __init__(self, graph, config):
        super().__init__(graph, config)
        self.graph_state_of = {}
        self.toks = _RecordingHashList(self.graph_state_of)
        self.toks.set_size(1000)

    def find_or_add_token(self, state, frame_plus_one, tot_cost):
        tok, changed = super().find_or_add_token(state, frame_plus_one, tot_cost)
        self.graph_state_of[tok.uid] = state
        return tok, changed

    def get_raw_lattice(self):
        """-> the lattice dict, or None where GetRawLattice has nothing to build (a frame without tokens)"""
        T = len(self.active_toks) - 1
        state_of, ordered = {}, []
        for f in range(T + 1):
            if not self.active_toks[f].toks:
                return None
            for t in self.top_sort_tokens(self.active_toks[f].toks):
                if t is not None:
                    state_of[t.uid] = len(ordered)
                    ordered.append((f, t))
        out = {k: [] for k in ops.FIELDS}
        use_final = bool(self.final_costs)
        for f, tok in ordered:
            out["frame"].append(f)
            out["graph_state"].append(self.graph_state_of[tok.uid])
            out["tot_cost"].append(tok.tot_cost)
            out["extra_cost"].append(tok.extra_cost)
            if f == T:
                out["final_cost"].append(self.final_costs.get(tok.uid, INF) if use_final else F(0.0))
            else:
                out["final_cost"].append(INF)
            out["arc_begin"].append(len(out["ilabel"]))
            for l in tok.links:
                out["ilabel"].append(l.ilabel)
                out["olabel"].append(l.olabel)
                out["graph_cost"].append(l.graph_cost)
                out["acoustic_cost"].append(F(l.acoustic_cost - self.cost_offsets[f]) if l.ilabel != 0 else F(0.0))
                out["nextstate"].append(state_of[l.next_tok.uid])
        out["arc_begin"].append(len(out["ilabel"]))
        lat = {k: np.asarray(v, np.int32 if k in ops.INTS else np.float32) for k, v in out.items()}
        lat["start"] = 0
        return lat


def rule_lattice(graph, config, ll, T, allow_partial=True):
    """DecodeUtteranceLatticeFaster (decoder-wrappers.cc:186-224) on a fresh decoder -> (lattice dict, result dict of
    lattice_faster_ref.decode_utterance_lattice_faster plus "weight", the best path's (Value1, Value2)).  The lattice is
    lattice_ops_ref.empty_lattice() unless the utterance succeeded."""
    dec = RawLatticeFasterDecoder(graph, config)
    out = dict(succeeded=False, partial=False, alignment=[], words=[], like=0.0, no_path=False, weight=None)
    if not dec.decode(ll, T):
        out["no_path"] = True
        return ops.empty_lattice(), out
    if not dec.reached_final():
        out["partial"] = True
        if not allow_partial:
            return ops.empty_lattice(), out
    ok, ali, words, w = dec.get_best_path()
    if not ok:
        out["no_path"] = True
        return ops.empty_lattice(), out
    out.update(succeeded=True, alignment=ali, words=words, like=float(F(-F(w[0] + w[1]))), weight=w)
    return dec.get_raw_lattice(), out


def same_lattice(got, want):
    """None, or the first field whose bytes differ (got: a khg.Lattice or a dict of arrays)"""
    for k in ops.FIELDS:
        g = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k))
        w = np.asarray(want[k])
        if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
            return k
    gs = got["start"] if isinstance(got, dict) else got.start
    return None if int(gs) == int(want["start"]) else "start"
