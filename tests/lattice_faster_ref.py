"""Plain-Python restatement of the reference's LatticeFasterDecoder + DecodeUtteranceLatticeFaster (the yardstick of the GPU tests).

Restates, line by line and in float32 (csrc/ of the reference):
  hash-list-inl.h                     HashList (bucket-ordered list; Insert = find-or-insert)
  lattice-faster-decoder.cc:61-98      InitDecoding / Decode
  :221-228                            PossiblyResizeHash
  :254-299                            FindOrAddToken
  :305-380                            PruneForwardLinks
  :386-472                            PruneForwardLinksFinal
  :492-548                            PruneTokensForFrame / PruneActiveTokens
  :551-588                            ComputeFinalCosts
  :591-653                            AdvanceDecoding / FinalizeDecoding
  :657-727                            GetCutoff (both branches)
  :730-825                            ProcessEmitting (best-token pre-pass, cost_offsets_)
  :840-905                            ProcessNonemitting (LIFO queue, links deleted on a re-visit)
  :935-1013                           TopSortTokens
  :101-192                            GetBestPath = GetRawLattice + OpenFst ShortestPath (n = 1)
  decoder-wrappers.cc:186-224         DecodeUtteranceLatticeFaster -> (succeeded, alignment, words, like)

Two choices are this file's own, written down in DESIGN.md: TopSortTokens walks its unordered_map in position order (the order of
token creation) and its reprocess set in insertion order; OpenFst's single-source ShortestPath on the top-sorted raw lattice visits
states in id order and replaces a predecessor only on a strictly better LatticeWeight (sum first, then graph cost).

It imports nothing from the package: numpy only."""
import numpy as np

F = np.float32
INF = F(np.inf)
INT32_MAX = 2 ** 31 - 1


class HashList:
    """hash-list-inl.h: one Elem per key; the list is "buckets in order of first occupation, insertion order inside a bucket"."""

    class Elem:
        __slots__ = ("key", "val", "tail")

    def __init__(self):
        self.list_head = None
        self.bucket_list_tail = -1
        self.hash_size = 0
        self.last_elem = []         # per bucket
        self.prev_bucket = []

    def set_size(self, size):
        self.hash_size = int(size)
        assert self.list_head is None and self.bucket_list_tail == -1
        if size > len(self.last_elem):
            self.last_elem += [None] * (size - len(self.last_elem))
            self.prev_bucket += [0] * (size - len(self.prev_bucket))

    def size(self):
        return self.hash_size

    def clear(self):
        b = self.bucket_list_tail
        while b != -1:
            self.last_elem[b] = None
            b = self.prev_bucket[b]
        self.bucket_list_tail = -1
        ans, self.list_head = self.list_head, None
        return ans

    def get_list(self):
        return self.list_head

    def _bucket_head(self, index):
        pb = self.prev_bucket[index]
        return self.list_head if pb == -1 else self.last_elem[pb].tail

    def find_elem(self, key):
        index = key % self.hash_size
        if self.last_elem[index] is None:
            return None
        e, tail = self._bucket_head(index), self.last_elem[index].tail
        while e is not tail:
            if e.key == key:
                return e
            e = e.tail
        return None

    def insert_elem(self, key, val):
        """-> (elem, is_new)"""
        index = key % self.hash_size
        if self.last_elem[index] is not None:
            e, tail = self._bucket_head(index), self.last_elem[index].tail
            while e is not tail:
                if e.key == key:
                    return e, False
                e = e.tail
        elem = HashList.Elem()
        elem.key, elem.val = key, val
        if self.last_elem[index] is None:
            if self.bucket_list_tail == -1:
                self.list_head = elem
            else:
                self.last_elem[self.bucket_list_tail].tail = elem
            elem.tail = None
            self.last_elem[index] = elem
            self.prev_bucket[index] = self.bucket_list_tail
            self.bucket_list_tail = index
        else:
            elem.tail = self.last_elem[index].tail
            self.last_elem[index].tail = elem
            self.last_elem[index] = elem
        return elem, True

    # the protocol of tests/golden/hashlist_ref_fresh.json (oracle/ref_hashlist_harness.cc)
    def insert(self, key, val):
        return self.insert_elem(key, val)[1]

    def put(self, key, val):
        e, _ = self.insert_elem(key, val)
        e.val = val

    def find(self, key):
        e = self.find_elem(key)
        return None if e is None else e.val

    def items(self):
        out, e = [], self.list_head
        while e is not None:
            out.append((e.key, e.val))
            e = e.tail
        return out

    def drop(self):
        self.clear()


class Token:
    __slots__ = ("tot_cost", "extra_cost", "links", "uid")

    def __init__(self, tot_cost, extra_cost, uid):
        self.tot_cost, self.extra_cost, self.links, self.uid = F(tot_cost), F(extra_cost), [], uid


class Link:                       # ForwardLink; a token's links are a Python list, head first
    __slots__ = ("next_tok", "ilabel", "olabel", "graph_cost", "acoustic_cost")

    def __init__(self, next_tok, ilabel, olabel, graph_cost, acoustic_cost):
        self.next_tok, self.ilabel, self.olabel = next_tok, ilabel, olabel
        self.graph_cost, self.acoustic_cost = F(graph_cost), F(acoustic_cost)


class TokenList:
    __slots__ = ("toks", "must_prune_forward_links", "must_prune_tokens")

    def __init__(self):
        self.toks = []            # creation order; the reference's singly linked list is this list reversed
        self.must_prune_forward_links = True
        self.must_prune_tokens = True


class Config:
    def __init__(self, beam=16.0, max_active=INT32_MAX, min_active=200, lattice_beam=10.0, prune_interval=25, beam_delta=0.5,
                 hash_ratio=2.0, prune_scale=0.1):
        self.beam, self.max_active, self.min_active = F(beam), int(max_active), int(min_active)
        self.lattice_beam, self.prune_interval, self.beam_delta = F(lattice_beam), int(prune_interval), F(beam_delta)
        self.hash_ratio, self.prune_scale = F(hash_ratio), F(prune_scale)


class Graph:
    """A StdVectorFst as CSR: out-arcs of state s are arc_off[s]:arc_off[s+1], in the order they were added."""

    def __init__(self, start, arc_off, ilabel, olabel, weight, nextstate, final):
        self.start = int(start)
        self.arc_off = [int(x) for x in arc_off]
        self.ilabel = [int(x) for x in ilabel]
        self.olabel = [int(x) for x in olabel]
        self.weight = [F(x) for x in weight]
        self.nextstate = [int(x) for x in nextstate]
        self.final = [F(x) for x in final]
        S = len(self.final)
        self.num_ieps = [sum(1 for a in range(self.arc_off[s], self.arc_off[s + 1]) if self.ilabel[a] == 0) for s in range(S)]

    @staticmethod
    def from_dict(d):
        return Graph(d["start"], d["arc_off"], d["ilabel"], d["olabel"], d["weight"], d["nextstate"], d["final"])

    def arcs(self, s):
        return range(self.arc_off[s], self.arc_off[s + 1])


def _approx_equal(a, b, tol):                          # kaldi-math.h:102-110
    if a == b:
        return True
    diff = abs(F(a - b))
    if diff == INF or diff != diff:
        return False
    return diff <= F(F(tol) * F(abs(a) + abs(b)))


class LatticeFasterDecoder:
    def __init__(self, graph: Graph, config: Config):
        self.fst, self.config = graph, config
        self.toks = HashList()
        self.toks.set_size(1000)                       # :36
        self.uid = 0

    # ---- search -------------------------------------------------------------------------------------------------------------
    def _new_token(self, tot_cost, extra_cost):
        self.uid += 1
        return Token(tot_cost, extra_cost, self.uid)

    def init_decoding(self):
        self.toks.clear()
        self.cost_offsets = []
        self.active_toks = [TokenList()]
        self.decoding_finalized = False
        self.final_costs = {}
        start_tok = self._new_token(0.0, 0.0)
        self.active_toks[0].toks.append(start_tok)
        self.toks.insert_elem(self.fst.start, start_tok)
        self.process_nonemitting(self.config.beam)

    def num_frames_decoded(self):
        return len(self.active_toks) - 1

    def decode(self, ll, T):
        """ll(frame, ilabel) -> float32 (the decodable's LogLikelihood, already scaled)."""
        self.init_decoding()
        while self.num_frames_decoded() < T:
            if self.num_frames_decoded() % self.config.prune_interval == 0:
                self.prune_active_tokens(F(self.config.lattice_beam * self.config.prune_scale))
            cost_cutoff = self.process_emitting(ll)
            self.process_nonemitting(cost_cutoff)
        self.finalize_decoding()
        return len(self.active_toks) > 0 and len(self.active_toks[-1].toks) > 0

    def possibly_resize_hash(self, num_toks):
        new_sz = int(F(F(num_toks) * self.config.hash_ratio))
        if new_sz > self.toks.size():
            self.toks.set_size(new_sz)

    def find_or_add_token(self, state, frame_plus_one, tot_cost):
        """-> (token, changed)"""
        e, is_new = self.toks.insert_elem(state, None)
        if is_new:
            tok = self._new_token(tot_cost, 0.0)
            self.active_toks[frame_plus_one].toks.append(tok)
            e.val = tok
            return tok, True
        tok = e.val
        if tok.tot_cost > tot_cost:
            tok.tot_cost = F(tot_cost)
            return tok, True
        return tok, False

    def get_cutoff(self, list_head):
        """-> (cutoff, tok_count, adaptive_beam, best_elem)"""
        c = self.config
        best_weight, best_elem, count = INF, None, 0
        if c.max_active == INT32_MAX and c.min_active == 0:
            e = list_head
            while e is not None:
                w = e.val.tot_cost
                if w < best_weight:
                    best_weight, best_elem = w, e
                e, count = e.tail, count + 1
            return F(best_weight + c.beam), count, c.beam, best_elem
        tmp = []
        e = list_head
        while e is not None:
            w = e.val.tot_cost
            tmp.append(w)
            if w < best_weight:
                best_weight, best_elem = w, e
            e, count = e.tail, count + 1
        beam_cutoff, min_active_cutoff, max_active_cutoff = F(best_weight + c.beam), INF, INF
        srt = sorted(tmp)                      # nth_element's k-th value == the k-th order statistic
        if len(tmp) > c.max_active:
            max_active_cutoff = srt[c.max_active]
        if max_active_cutoff < beam_cutoff:
            return max_active_cutoff, count, F(F(max_active_cutoff - best_weight) + c.beam_delta), best_elem
        if len(tmp) > c.min_active:
            min_active_cutoff = best_weight if c.min_active == 0 else srt[c.min_active]
        if min_active_cutoff > beam_cutoff:
            return min_active_cutoff, count, F(F(min_active_cutoff - best_weight) + c.beam_delta), best_elem
        return beam_cutoff, count, c.beam, best_elem

    def process_emitting(self, ll):
        frame = len(self.active_toks) - 1
        self.active_toks.append(TokenList())
        final_toks = self.toks.clear()
        cur_cutoff, tok_cnt, adaptive_beam, best_elem = self.get_cutoff(final_toks)
        self.possibly_resize_hash(tok_cnt)
        next_cutoff = INF
        cost_offset = F(0.0)
        fst = self.fst
        if best_elem is not None:
            tok = best_elem.val
            cost_offset = F(-tok.tot_cost)
            for a in fst.arcs(best_elem.key):
                if fst.ilabel[a] != 0:
                    new_weight = F(F(F(fst.weight[a] + cost_offset) - ll(frame, fst.ilabel[a])) + tok.tot_cost)
                    if F(new_weight + adaptive_beam) < next_cutoff:
                        next_cutoff = F(new_weight + adaptive_beam)
        while len(self.cost_offsets) < frame + 1:
            self.cost_offsets.append(F(0.0))
        self.cost_offsets[frame] = cost_offset
        e = final_toks
        while e is not None:
            tok = e.val
            if tok.tot_cost <= cur_cutoff:
                for a in fst.arcs(e.key):
                    if fst.ilabel[a] != 0:
                        ac_cost = F(cost_offset - ll(frame, fst.ilabel[a]))
                        graph_cost = fst.weight[a]
                        tot_cost = F(F(tok.tot_cost + ac_cost) + graph_cost)
                        if tot_cost >= next_cutoff:
                            continue
                        elif F(tot_cost + adaptive_beam) < next_cutoff:
                            next_cutoff = F(tot_cost + adaptive_beam)
                        next_tok, _ = self.find_or_add_token(fst.nextstate[a], frame + 1, tot_cost)
                        tok.links.insert(0, Link(next_tok, fst.ilabel[a], fst.olabel[a], graph_cost, ac_cost))
            e = e.tail
        return next_cutoff

    def process_nonemitting(self, cutoff):
        fst = self.fst
        queue = []
        e = self.toks.get_list()
        while e is not None:
            if fst.num_ieps[e.key] != 0:
                queue.append(e)
            e = e.tail
        while queue:
            e = queue.pop()
            tok = e.val
            cur_cost = tok.tot_cost
            if cur_cost >= cutoff:
                continue
            tok.links = []                             # DeleteForwardLinks: necessary when re-visiting
            for a in fst.arcs(e.key):
                if fst.ilabel[a] == 0:
                    graph_cost = fst.weight[a]
                    tot_cost = F(cur_cost + graph_cost)
                    if tot_cost < cutoff:
                        ns = fst.nextstate[a]
                        e_new, _ = self.toks.insert_elem(ns, None)
                        # FindOrAddToken through the same Elem (the hash lookup above is the one FindOrAddToken does)
                        if e_new.val is None:
                            nt = self._new_token(tot_cost, 0.0)
                            self.active_toks[-1].toks.append(nt)
                            e_new.val, changed = nt, True
                        elif e_new.val.tot_cost > tot_cost:
                            e_new.val.tot_cost, changed = tot_cost, True
                        else:
                            changed = False
                        tok.links.insert(0, Link(e_new.val, 0, fst.olabel[a], graph_cost, 0.0))
                        if changed and fst.num_ieps[ns] != 0:
                            queue.append(e_new)

    # ---- pruning ------------------------------------------------------------------------------------------------------------
    def prune_forward_links(self, f, delta):
        extra_costs_changed = links_pruned = False
        lattice_beam = self.config.lattice_beam
        changed = True
        with np.errstate(invalid="ignore"):
            while changed:
                changed = False
                for tok in reversed(self.active_toks[f].toks):
                    tok_extra_cost = INF
                    kept = []
                    for link in tok.links:
                        nt = link.next_tok
                        lec = F(nt.extra_cost + F(F(F(tok.tot_cost + link.acoustic_cost) + link.graph_cost) - nt.tot_cost))
                        if lec > lattice_beam:
                            links_pruned = True
                        else:
                            if lec < 0.0:
                                lec = F(0.0)
                            if lec < tok_extra_cost:
                                tok_extra_cost = lec
                            kept.append(link)
                    tok.links = kept
                    if abs(F(tok_extra_cost - tok.extra_cost)) > delta:
                        changed = True
                    tok.extra_cost = tok_extra_cost
                if changed:
                    extra_costs_changed = True
        return extra_costs_changed, links_pruned

    def prune_tokens_for_frame(self, f):
        self.active_toks[f].toks = [t for t in self.active_toks[f].toks if t.extra_cost != INF]

    def prune_active_tokens(self, delta):
        cur = self.num_frames_decoded()
        for f in range(cur - 1, -1, -1):
            at = self.active_toks[f]
            if at.must_prune_forward_links:
                ecc, lp = self.prune_forward_links(f, delta)
                if ecc and f > 0:
                    self.active_toks[f - 1].must_prune_forward_links = True
                if lp:
                    at.must_prune_tokens = True
                at.must_prune_forward_links = False
            if f + 1 < cur and self.active_toks[f + 1].must_prune_tokens:
                self.prune_tokens_for_frame(f + 1)
                self.active_toks[f + 1].must_prune_tokens = False

    def compute_final_costs(self):
        """-> (final_costs {uid: cost}, final_relative_cost, final_best_cost)"""
        final_costs = {}
        best_cost = best_cost_with_final = INF
        e = self.toks.get_list()
        while e is not None:
            final_cost = self.fst.final[e.key]
            tok = e.val
            cost = tok.tot_cost
            cost_with_final = F(cost + final_cost)
            best_cost = min(cost, best_cost)
            best_cost_with_final = min(cost_with_final, best_cost_with_final)
            if final_cost != INF:
                final_costs[tok.uid] = final_cost
            e = e.tail
        rel = INF if (best_cost == INF and best_cost_with_final == INF) else F(best_cost_with_final - best_cost)
        best = best_cost_with_final if best_cost_with_final != INF else best_cost
        return final_costs, rel, best

    def prune_forward_links_final(self):
        f = len(self.active_toks) - 1
        self.final_costs, self.final_relative_cost, self.final_best_cost = self.compute_final_costs()
        self.decoding_finalized = True
        self.toks.clear()
        lattice_beam = self.config.lattice_beam
        changed = True
        with np.errstate(invalid="ignore"):
            while changed:
                changed = False
                for tok in reversed(self.active_toks[f].toks):
                    if not self.final_costs:
                        final_cost = F(0.0)
                    else:
                        final_cost = self.final_costs.get(tok.uid, INF)
                    tok_extra_cost = F(F(tok.tot_cost + final_cost) - self.final_best_cost)
                    kept = []
                    for link in tok.links:
                        nt = link.next_tok
                        lec = F(nt.extra_cost + F(F(F(tok.tot_cost + link.acoustic_cost) + link.graph_cost) - nt.tot_cost))
                        if lec > lattice_beam:
                            continue
                        if lec < 0.0:
                            lec = F(0.0)
                        if lec < tok_extra_cost:
                            tok_extra_cost = lec
                        kept.append(link)
                    tok.links = kept
                    if tok_extra_cost > lattice_beam:
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

    def reached_final(self):
        return self.final_relative_cost != INF

    # ---- best path ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def top_sort_tokens(toks):
        """toks in creation order -> topsorted list (None in the gaps)."""
        num = len(toks)
        pos = {t.uid: i for i, t in enumerate(toks)}        # list head (newest) gets num - 1 ... oldest 0
        by_uid = {t.uid: t for t in toks}
        cur_pos = num
        reprocess = {}                                      # insertion-ordered set

        def visit(tok):
            nonlocal cur_pos
            p = pos[tok.uid]
            for link in tok.links:
                if link.ilabel == 0 and link.next_tok.uid in pos:
                    if pos[link.next_tok.uid] < p:
                        pos[link.next_tok.uid] = cur_pos
                        cur_pos += 1
                        reprocess[link.next_tok.uid] = True
        for t in toks:
            visit(t)
            reprocess.pop(t.uid, None)
        loops = 0
        while reprocess and loops < 1000000:
            vec = list(reprocess)
            reprocess.clear()
            for uid in vec:
                visit(by_uid[uid])
            loops += 1
        assert loops < 1000000, "Epsilon loops exist in your decoding graph"
        out = [None] * cur_pos
        for uid, p in pos.items():
            out[p] = by_uid[uid]
        return out

    def get_best_path(self):
        """GetRawLattice + ShortestPath + GetLinearSymbolSequence -> (ok, alignment, words, (value1, value2))."""
        num_frames = len(self.active_toks) - 1
        state_of, ordered = {}, []
        for f in range(num_frames + 1):
            if not self.active_toks[f].toks:
                return False, [], [], None
            for t in self.top_sort_tokens(self.active_toks[f].toks):
                if t is not None:
                    state_of[t.uid] = len(ordered)
                    ordered.append((f, t))
        n = len(ordered)
        arcs = [[] for _ in range(n)]
        final = [None] * n
        use_final = bool(self.final_costs)
        for f in range(num_frames + 1):
            for tok in reversed(self.active_toks[f].toks):
                s = state_of[tok.uid]
                for l in tok.links:
                    off = self.cost_offsets[f] if l.ilabel != 0 else F(0.0)
                    arcs[s].append((l.ilabel, l.olabel, l.graph_cost, F(l.acoustic_cost - off), state_of[l.next_tok.uid]))
                if f == num_frames:
                    if use_final:
                        if tok.uid in self.final_costs:
                            final[s] = (self.final_costs[tok.uid], F(0.0))
                    else:
                        final[s] = (F(0.0), F(0.0))
        return shortest_path(arcs, final)


def natural_less(a, b):
    """Kaldi LatticeWeight: a strictly better than b (Compare(a, b) == 1)."""
    fa, fb = F(a[0] + a[1]), F(b[0] + b[1])
    if fa < fb:
        return True
    if fa > fb:
        return False
    return a[0] < b[0]


def shortest_path(arcs, final):
    """OpenFst SingleShortestPath on a top-sorted acyclic lattice from state 0 (StateOrderQueue): states in id order; a distance
    (and parent) changes only on a strictly better weight; then GetLinearSymbolSequence along the path."""
    n = len(arcs)
    if n == 0:
        return False, [], [], None
    dist = [None] * n
    parent = [None] * n
    dist[0] = (F(0.0), F(0.0))
    f_dist, f_parent = None, -1
    for s in range(n):
        sd = dist[s]
        if sd is None:
            continue
        if final[s] is not None:
            w = (F(sd[0] + final[s][0]), F(sd[1] + final[s][1]))
            if f_dist is None or natural_less(w, f_dist):
                f_dist, f_parent = w, s
        for i, (il, ol, g, ac, ns) in enumerate(arcs[s]):
            w = (F(sd[0] + g), F(sd[1] + ac))
            if dist[ns] is None or natural_less(w, dist[ns]):
                dist[ns] = w
                parent[ns] = (s, i)
    if f_parent < 0:
        return False, [], [], None
    path = []
    s = f_parent
    while s != 0:
        p, i = parent[s]
        path.append(arcs[p][i])
        s = p
    path.reverse()
    v1, v2 = F(0.0), F(0.0)
    ali, words = [], []
    for il, ol, g, ac, ns in path:
        v1, v2 = F(g + v1), F(ac + v2)
        if il != 0:
            ali.append(il)
        if ol != 0:
            words.append(ol)
    v1, v2 = F(final[f_parent][0] + v1), F(final[f_parent][1] + v2)
    return True, ali, words, (v1, v2)


def decode_utterance_lattice_faster(graph: Graph, config: Config, ll, T, allow_partial=True):
    """decoder-wrappers.cc:186-224 on a fresh decoder -> dict(succeeded, partial, alignment, words, like, no_path).
    like = -(value1 + value2) in float, returned as the double it converts to."""
    dec = LatticeFasterDecoder(graph, config)
    out = dict(succeeded=False, partial=False, alignment=[], words=[], like=0.0, no_path=False)
    if not dec.decode(ll, T):
        out["no_path"] = True
        return out
    if not dec.reached_final():
        out["partial"] = True
        if not allow_partial:
            return out
    ok, ali, words, w = dec.get_best_path()
    if not ok:
        out["no_path"] = True           # the reference raises here ("Failed to get traceback")
        return out
    out.update(succeeded=True, alignment=ali, words=words, like=float(F(-F(w[0] + w[1]))))
    return out


def score_fn(loglikes, pdfs, id2pdf, acoustic_scale):
    """K1's per-utterance [npdf][T] matrix (return_scores) -> ll(frame, tid) = float32(acoustic_scale * loglike), the
    DecodableAmDiagGmmScaled::LogLikelihood of decodable-am-diag-gmm.h."""
    col = {int(p): j for j, p in enumerate(pdfs)}
    m = np.asarray(loglikes, np.float32)
    sc = F(acoustic_scale)

    def ll(frame, tid):
        return F(sc * m[col[int(id2pdf[tid])], frame])
    return ll
