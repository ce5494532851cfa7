"""Plain-Python restatement of the reference's LatticeSimpleDecoder + DecodeUtteranceLatticeSimple (the yardstick of
tests/test_gpu_lattice_simple.py).

Restates, line by line and in float32 (csrc/ of the reference):
  lattice-simple-decoder.cc:40-66      InitDecoding
  :68-142                             ProcessNonemitting (LIFO queue, links deleted on a re-visit; Quirk 1 raises)
  :144-165                            Decode (returns !final_costs_.empty())
  :174-219                            FindOrAddToken
  :224-309                            PruneForwardLinks (the NaN check of :261 raises)
  :314-342                            PruneTokensForFrame
  :349-383                            PruneActiveTokens
  :385-426                            ProcessEmitting (running cutoff)
  :431-461                            PruneCurrentTokens (best starts at 1e10)
  :466-582                            FinalizeDecoding / PruneForwardLinksFinal (ApproxEqual 1e-5)
  :584-628                            ComputeFinalCosts
  :644-735                            GetBestPath = GetRawLattice + ShortestPath
  decoder-wrappers.cc:142-182         DecodeUtteranceLatticeSimple -> (succeeded, alignment, words, like)

The reference walks std::unordered_maps; `walk` picks the order here: "insertion", "reversed" or "shuffle" (seeded), so a test can
show that the answer does not depend on it.  ShortestPath follows the tie rule of the GPU kernel: frame by
frame, emitting in-links first, then epsilon in-links in Jacobi rounds; a destination takes its in-links ordered by (source state,
arc index) and changes only on a strictly better LatticeWeight; the final state is the lowest one among exact ties.

A negative-cost epsilon cycle, on which the reference never returns, raises EpsilonLoop: the closure raises once it has run long
(more pops than 4 (S + 2)^2 + 1000) on a graph whose epsilon arcs hold a negative cycle (Bellman-Ford in float64); on a graph without
one it runs on, however long, as the reference does.  `stats` (a dict, optional) receives what FinalizeDecoding left: surviving
tokens, those with a nonzero extra cost, and links excised by lattice_beam.  Imports Graph and score_fn from lattice_faster_ref;
numpy only otherwise."""
import random

import numpy as np

from lattice_faster_ref import Graph, _approx_equal, score_fn  # noqa: F401

F = np.float32
INF = F(np.inf)


class DecodeError(RuntimeError):
    """What the reference throws (KHG_ERR / KHG_ASSERT), with its message."""


class EpsilonLoop(DecodeError):
    """A negative-cost epsilon cycle: the reference's ProcessNonemitting never ends."""


class Config:
    def __init__(self, beam=16.0, lattice_beam=10.0, prune_interval=25, prune_scale=0.1):
        self.beam, self.lattice_beam, self.prune_interval, self.prune_scale = F(beam), F(lattice_beam), int(prune_interval), F(prune_scale)


class Token:
    __slots__ = ("tot_cost", "extra_cost", "links", "state", "uid")

    def __init__(self, tot_cost, state, uid):
        self.tot_cost, self.extra_cost, self.links, self.state, self.uid = F(tot_cost), F(0.0), [], state, uid


class Link:                       # ForwardLink; a token's links are a Python list, head first
    __slots__ = ("next_tok", "ilabel", "olabel", "graph_cost", "acoustic_cost", "arc")

    def __init__(self, next_tok, ilabel, olabel, graph_cost, acoustic_cost, arc):
        self.next_tok, self.ilabel, self.olabel = next_tok, ilabel, olabel
        self.graph_cost, self.acoustic_cost, self.arc = F(graph_cost), F(acoustic_cost), arc


def _min(a, b):                   # std::min(a, b)
    return b if b < a else a


def has_negative_eps_cycle(g: Graph):
    """Bellman-Ford in float64 over the input-epsilon arcs, every state a source: a relaxation after S rounds means a negative cycle."""
    S = len(g.final)
    d = [0.0] * S
    eps = [(s, g.nextstate[a], float(g.weight[a])) for s in range(S) for a in g.arcs(s) if g.ilabel[a] == 0]
    for _ in range(S + 1):
        changed = False
        for s, n, w in eps:
            if d[s] + w < d[n]:
                d[n] = d[s] + w
                changed = True
        if not changed:
            return False
    return True


class LatticeSimpleDecoder:
    def __init__(self, graph: Graph, config: Config, walk="insertion", seed=0):
        assert walk in ("insertion", "reversed", "shuffle")
        self.fst, self.config, self.walk_kind, self.rng = graph, config, walk, random.Random(seed)
        self.uid = 0
        self.excised = 0                 # links excised by lattice_beam (interval and final pruning)
        self.neg_cycle = None

    def walk(self, d):
        keys = list(d.keys())
        if self.walk_kind == "reversed":
            keys.reverse()
        elif self.walk_kind == "shuffle":
            self.rng.shuffle(keys)
        return keys

    def init_decoding(self):
        self.cur_toks, self.prev_toks = {}, {}
        self.final_costs = {}
        self.decoding_finalized = False
        self.active_toks = [[]]          # per frame: tokens, the list head LAST; must_prune flags alongside
        self.must_prune = [[True, True]]
        start_tok = self._new_token(0.0, self.fst.start)
        self.active_toks[0].append(start_tok)
        self.cur_toks[self.fst.start] = start_tok
        self.process_nonemitting()

    def _new_token(self, tot_cost, state):
        self.uid += 1
        return Token(tot_cost, state, self.uid)

    def num_frames_decoded(self):
        return len(self.active_toks) - 1

    def process_nonemitting(self):
        frame = len(self.active_toks) - 2
        queue = []
        best_cost = INF
        for s in self.walk(self.cur_toks):
            if self.fst.num_ieps[s] != 0:
                queue.append(s)
            best_cost = _min(best_cost, self.cur_toks[s].tot_cost)
        if not queue:
            raise DecodeError("Error in ProcessNonEmitting: no surviving tokens: frame is %d" % frame)
        cutoff = F(best_cost + self.config.beam)
        S = len(self.fst.final)
        pops, cap = 0, 4 * (S + 2) * (S + 2) + 1000
        while queue:
            pops += 1
            if pops > cap:
                if self.neg_cycle is None:
                    self.neg_cycle = has_negative_eps_cycle(self.fst)
                if self.neg_cycle:
                    raise EpsilonLoop("negative-cost epsilon cycle at frame %d" % frame)
            state = queue.pop()
            tok = self.cur_toks[state]
            tok.links = []
            for a in self.fst.arcs(state):
                if self.fst.ilabel[a] == 0:
                    graph_cost = self.fst.weight[a]
                    tot_cost = F(tok.tot_cost + graph_cost)
                    if tot_cost < cutoff:
                        ns = self.fst.nextstate[a]
                        new_tok, changed = self.find_or_add_token(ns, frame + 1, tot_cost)
                        tok.links.insert(0, Link(new_tok, 0, self.fst.olabel[a], graph_cost, 0.0, a))
                        if changed and self.fst.num_ieps[ns] != 0:
                            queue.append(ns)

    def find_or_add_token(self, state, frame, tot_cost):
        tok = self.cur_toks.get(state)
        if tok is None:
            tok = self._new_token(tot_cost, state)
            self.active_toks[frame].append(tok)
            self.cur_toks[state] = tok
            return tok, True
        if tok.tot_cost > tot_cost:
            tok.tot_cost = F(tot_cost)
            return tok, True
        return tok, False

    def decode(self, ll, T):
        """ll(frame, ilabel) -> float32 (the decodable's LogLikelihood); T frames (IsLastFrame(t) == (t == T - 1))."""
        self.init_decoding()
        while self.num_frames_decoded() - 1 != T - 1:
            if self.num_frames_decoded() % self.config.prune_interval == 0:
                self.prune_active_tokens(F(self.config.lattice_beam * self.config.prune_scale))
            self.process_emitting(ll)
            self.prune_current_tokens()
            self.process_nonemitting()
        self.finalize_decoding()
        return len(self.final_costs) > 0

    def process_emitting(self, ll):
        frame = len(self.active_toks) - 1
        self.active_toks.append([])
        self.must_prune.append([True, True])
        self.prev_toks, self.cur_toks = self.cur_toks, {}
        cutoff = INF
        for state in self.walk(self.prev_toks):
            tok = self.prev_toks[state]
            for a in self.fst.arcs(state):
                il = self.fst.ilabel[a]
                if il != 0:
                    ac_cost = F(-ll(frame, il))
                    graph_cost = self.fst.weight[a]
                    tot_cost = F(F(tok.tot_cost + ac_cost) + graph_cost)
                    if tot_cost >= cutoff:
                        continue
                    elif F(tot_cost + self.config.beam) < cutoff:
                        cutoff = F(tot_cost + self.config.beam)
                    next_tok, _ = self.find_or_add_token(self.fst.nextstate[a], frame + 1, tot_cost)
                    tok.links.insert(0, Link(next_tok, il, self.fst.olabel[a], graph_cost, ac_cost, a))

    def prune_current_tokens(self):
        toks = self.cur_toks
        if not toks:
            return
        best_cost = F(1.0e10)
        for s in self.walk(toks):
            best_cost = _min(best_cost, toks[s].tot_cost)
        cutoff = F(best_cost + self.config.beam)
        retained = [s for s in self.walk(toks) if toks[s].tot_cost < cutoff]
        self.cur_toks = {s: toks[s] for s in retained}

    def prune_forward_links(self, f, delta):
        extra_costs_changed = links_pruned = False
        changed = True
        lb = self.config.lattice_beam
        while changed:
            changed = False
            for tok in reversed(self.active_toks[f]):
                tok_extra_cost = INF
                kept = []
                for link in tok.links:
                    nt = link.next_tok
                    lec = F(nt.extra_cost + F(F(F(tok.tot_cost + link.acoustic_cost) + link.graph_cost) - nt.tot_cost))
                    if lec != lec:
                        raise DecodeError("Check failed!\nx: link_extra_cost == link_extra_cost")
                    if lec > lb:
                        links_pruned = True
                        self.excised += 1
                    else:
                        if lec < 0.0:
                            lec = F(0.0)
                        if lec < tok_extra_cost:
                            tok_extra_cost = lec
                        kept.append(link)
                tok.links = kept
                with np.errstate(invalid="ignore"):                # inf - inf: NaN, which is not > delta, as in C++
                    moved = abs(F(tok_extra_cost - tok.extra_cost)) > delta
                if moved:
                    changed = True
                tok.extra_cost = tok_extra_cost
            if changed:
                extra_costs_changed = True
        return extra_costs_changed, links_pruned

    def prune_tokens_for_frame(self, f):
        self.active_toks[f] = [t for t in self.active_toks[f] if t.extra_cost != INF]

    def prune_active_tokens(self, delta):
        cur_frame_plus_one = self.num_frames_decoded()
        for f in range(cur_frame_plus_one - 1, -1, -1):
            if self.must_prune[f][0]:
                ecc, lp = self.prune_forward_links(f, delta)
                if ecc and f > 0:
                    self.must_prune[f - 1][0] = True
                if lp:
                    self.must_prune[f][1] = True
                self.must_prune[f][0] = False
            if f + 1 < cur_frame_plus_one and self.must_prune[f + 1][1]:
                self.prune_tokens_for_frame(f + 1)
                self.must_prune[f + 1][1] = False

    def compute_final_costs(self):
        final_costs = {}
        best_cost = best_cost_with_final = INF
        for state in self.walk(self.cur_toks):
            tok = self.cur_toks[state]
            final_cost = self.fst.final[state]
            cost = tok.tot_cost
            cost_with_final = F(cost + final_cost)
            best_cost = _min(cost, best_cost)
            best_cost_with_final = _min(cost_with_final, best_cost_with_final)
            if final_cost != INF:
                final_costs[tok.uid] = final_cost
        if best_cost == INF and best_cost_with_final == INF:
            final_relative_cost = INF
        else:
            final_relative_cost = F(best_cost_with_final - best_cost)
        final_best_cost = best_cost_with_final if best_cost_with_final != INF else best_cost
        return final_costs, final_relative_cost, final_best_cost

    def prune_forward_links_final(self):
        fpo = len(self.active_toks) - 1
        self.final_costs, self.final_relative_cost, self.final_best_cost = self.compute_final_costs()
        self.decoding_finalized = True
        self.cur_toks = {}
        lb = self.config.lattice_beam
        changed = True
        while changed:
            changed = False
            for tok in reversed(self.active_toks[fpo]):
                if not self.final_costs:
                    final_cost = F(0.0)
                else:
                    final_cost = self.final_costs.get(tok.uid, INF)
                tok_extra_cost = F(F(tok.tot_cost + final_cost) - self.final_best_cost)
                kept = []
                for link in tok.links:
                    nt = link.next_tok
                    lec = F(nt.extra_cost + F(F(F(tok.tot_cost + link.acoustic_cost) + link.graph_cost) - nt.tot_cost))
                    if lec > lb:
                        self.excised += 1
                        continue
                    if lec < 0.0:
                        lec = F(0.0)
                    if lec < tok_extra_cost:
                        tok_extra_cost = lec
                    kept.append(link)
                tok.links = kept
                if tok_extra_cost > lb:
                    tok_extra_cost = INF
                if not _approx_equal(tok.extra_cost, tok_extra_cost, 1.0e-05):
                    changed = True
                tok.extra_cost = tok_extra_cost

    def finalize_decoding(self):
        final_frame_plus_one = self.num_frames_decoded()
        self.prune_forward_links_final()
        for f in range(final_frame_plus_one - 1, -1, -1):
            self.prune_forward_links(f, F(0.0))
            self.prune_tokens_for_frame(f + 1)
        self.prune_tokens_for_frame(0)

    def get_best_path(self):
        """GetRawLattice + ShortestPath (the kernel's tie rule) + GetLinearSymbolSequence -> (ok, alignment, words, (v1, v2))."""
        T = self.num_frames_decoded()
        if not T > 0:
            raise DecodeError("Check failed!\nx: num_frames > 0")
        if any(not self.active_toks[f] for f in range(T + 1)):
            return False, [], [], None
        by_state = []
        for f in range(T + 1):
            d = {}
            for tok in self.active_toks[f]:
                assert tok.state not in d, "two surviving tokens of one state on a frame"
                d[tok.state] = tok
            by_state.append(d)
        # in-links of every surviving token, (source state, arc index) order
        inl = []
        for f in range(T + 1):
            e = {}
            for tok in self.active_toks[f]:
                for link in tok.links:
                    nf = f + 1 if link.ilabel != 0 else f
                    e.setdefault((nf, link.next_tok.uid), []).append((tok.state, link.arc, tok, link))
            for v in e.values():
                v.sort(key=lambda x: (x[0], x[1]))
            inl.append(e)

        def links_into(f, tok, emitting):
            out = []
            for src_f in ((f - 1,) if emitting else (f,)):
                if src_f < 0:
                    continue
                for c in inl[src_f].get((f, tok.uid), []):
                    if (c[3].ilabel != 0) == emitting:
                        out.append(c)
            out.sort(key=lambda x: (x[0], x[1]))
            return out

        def less(a, b):
            fa, fb = F(a[0] + a[1]), F(b[0] + b[1])
            if fa < fb:
                return True
            if fa > fb:
                return False
            return a[0] < b[0]

        S = len(self.fst.final)
        dist = []       # per frame: state -> (v1, v2, back-pointer (src frame, src state, link) or None)
        for f in range(T + 1):
            toks = sorted(by_state[f].items())
            P = {}
            if f == 0:
                st = by_state[0].get(self.fst.start)
                if st is not None:
                    P[self.fst.start] = (F(0.0), F(0.0), None)
            else:
                prev = dist[f - 1]
                for s, tok in toks:
                    for src, _, stok, link in links_into(f, tok, True):
                        if src not in prev:
                            continue
                        c = (F(prev[src][0] + link.graph_cost), F(prev[src][1] + link.acoustic_cost))
                        if s not in P or less(c, P[s]):
                            P[s] = (c[0], c[1], (f - 1, src, link))
            for rnd in range(S + 2):
                new = dict(P)
                changed = False
                for s, tok in toks:
                    for src, _, stok, link in links_into(f, tok, False):
                        if src not in P:
                            continue
                        c = (F(P[src][0] + link.graph_cost), F(P[src][1] + F(0.0)))
                        if s not in new or less(c, new[s]):
                            new[s] = (c[0], c[1], (f, src, link))
                            changed = True
                P = new
                if not changed:
                    break
            else:
                raise EpsilonLoop("no fixpoint of the best-path epsilon rounds")
            dist.append(P)
        best, fp = None, None
        for s, tok in sorted(by_state[T].items()):
            if s not in dist[T] or tok.uid not in self.final_costs:
                continue
            w = (F(dist[T][s][0] + self.final_costs[tok.uid]), F(dist[T][s][1] + F(0.0)))
            if best is None or less(w, best):
                best, fp = w, s
        if fp is None:
            return False, [], [], None
        ali, words = [], []
        f, s = T, fp
        while dist[f][s][2] is not None:
            pf, ps, link = dist[f][s][2]
            if link.ilabel != 0:
                ali.append(link.ilabel)
            if link.olabel != 0:
                words.append(link.olabel)
            f, s = pf, ps
        ali.reverse()
        words.reverse()
        return True, ali, words, best


def decode_utterance_lattice_simple(graph: Graph, config: Config, ll, T, allow_partial=True, walk="insertion", seed=0, stats=None):
    """decoder-wrappers.cc:142-182 on a fresh decoder -> dict(succeeded, alignment, words, like); raises DecodeError where the
    reference throws.  like = -(value1 + value2) in float, returned as the double it converts to.  allow_partial never matters:
    Decode() is false whenever no final state is live at the end (Quirk 2)."""
    dec = LatticeSimpleDecoder(graph, config, walk, seed)
    out = dict(succeeded=False, alignment=[], words=[], like=0.0)
    decoded = dec.decode(ll, T)
    if stats is not None:
        toks = [t for frame in dec.active_toks for t in frame]
        stats["tokens"] = stats.get("tokens", 0) + len(toks)
        stats["nonzero_extra"] = stats.get("nonzero_extra", 0) + sum(1 for t in toks if t.extra_cost != 0.0)
        stats["excised"] = stats.get("excised", 0) + dec.excised
    if not decoded:
        return out
    ok, ali, words, w = dec.get_best_path()
    if not ok:
        raise DecodeError("Failed to get traceback")
    out.update(succeeded=True, alignment=ali, words=words, like=float(F(-F(w[0] + w[1]))))
    return out


def add_eps_self_loops(g, weight=0.0):
    """A copy of a graph dict with an input-epsilon self-loop (0:0/weight) after the arcs of every state.  At weight 0 no path's
    weight changes, and every live token has an input-epsilon arc, so Quirk 1 never fires; it also pins every extra cost at 0 (the
    loop's link extra cost is the token's own, which starts at 0).  A positive weight keeps the extra costs free."""
    S = len(g["final"])
    arc_off = [int(x) for x in g["arc_off"]]
    il, ol, w, ns = [], [], [], []
    new_off = [0]
    for s in range(S):
        for a in range(arc_off[s], arc_off[s + 1]):
            il.append(int(g["ilabel"][a])); ol.append(int(g["olabel"][a])); w.append(float(g["weight"][a])); ns.append(int(g["nextstate"][a]))
        il.append(0); ol.append(0); w.append(float(weight)); ns.append(s)
        new_off.append(len(il))
    return {"start": int(g["start"]), "arc_off": np.asarray(new_off, np.int64), "ilabel": np.asarray(il, np.int32),
            "olabel": np.asarray(ol, np.int32), "weight": np.asarray(w, np.float32), "nextstate": np.asarray(ns, np.int32),
            "final": np.asarray(g["final"], np.float32)}


def matrix_ll(m):
    """DecodableCtc / a matrix decodable: ll(frame, index) = m[frame, index - 1]."""
    m = np.asarray(m, np.float32)

    def ll(frame, index):
        return F(m[frame, index - 1])
    return ll
