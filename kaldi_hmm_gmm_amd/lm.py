"""Backoff n-gram language models for lattice-lmrescore: the automaton of khg_lm_create (include/khg_hip.h) as numpy
arrays (NgramLm), read from ARPA text (NgramLm.from_arpa), made from the word probabilities of a word-loop graph (NgramLm.unigram) or
estimated from transcripts (estimate_ngram_lm).  DeviceLm(lm, ctx) uploads one; DeviceLattices.lm_rescore and Lattice.lm_rescore use it.

The automaton: state 0 is the empty history, `start` the history <s>; state h owns the arcs arc_begin[h] .. arc_begin[h + 1] (word
ascending, cost = -ln P, next); a word that h does not list costs backoff_cost[h] more and is looked up in backoff[h] (< h);
final_cost[h] is the cost of the sentence end from h."""
import math
from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import KhgError

_BOS = 0        # <s> inside a history tuple: it sorts before every word (word-ids are > 0)


class NgramLm:
    """A deterministic backoff automaton in flat arrays; validated by khg_lm_validate."""

    def __init__(self, backoff, backoff_cost, arc_begin, word, cost, next, final_cost, start: int):
        self.backoff = _lib.as_np(backoff, np.int32)
        self.backoff_cost = _lib.as_np(backoff_cost, np.float32)
        self.arc_begin = _lib.as_np(arc_begin, np.int32)
        self.word = _lib.as_np(word, np.int32)
        self.cost = _lib.as_np(cost, np.float32)
        self.next = _lib.as_np(next, np.int32)
        self.final_cost = _lib.as_np(final_cost, np.float32)
        self.start = int(start)
        n = self.backoff.shape[0]
        if (self.backoff.ndim != 1 or n < 1 or self.backoff_cost.shape != (n,) or self.final_cost.shape != (n,)
                or self.arc_begin.shape != (n + 1,)):
            raise KhgError("khg_lm_validate: one backoff, backoff_cost and final_cost per state, one arc_begin more")
        if self.arc_begin[0] != 0 or (np.diff(self.arc_begin) < 0).any():
            raise KhgError("khg_lm_validate: arc_begin must run from 0, monotone")
        a = int(self.arc_begin[n])
        if self.word.shape != (a,) or self.cost.shape != (a,) or self.next.shape != (a,):
            raise KhgError("khg_lm_validate: one word, cost and next per arc")
        _lib.check(_lib.lib.khg_lm_validate(*self._c_args()))

    def _c_args(self):
        i32, f32 = _lib.C.c_int32, _lib.C.c_float
        return (self.num_states, _lib.ptr(self.backoff, i32), _lib.ptr(self.backoff_cost, f32), _lib.ptr(self.arc_begin, i32),
                _lib.ptr(self.word, i32), _lib.ptr(self.cost, f32), _lib.ptr(self.next, i32), _lib.ptr(self.final_cost, f32), self.start)

    @property
    def num_states(self) -> int:
        return int(self.backoff.shape[0])

    @property
    def num_arcs(self) -> int:
        return int(self.word.shape[0])

    def to_arrays(self) -> dict:
        return {"backoff": self.backoff, "backoff_cost": self.backoff_cost, "arc_begin": self.arc_begin, "word": self.word,
                "cost": self.cost, "next": self.next, "final_cost": self.final_cost, "start": self.start}

    def score(self, words: Sequence[int]) -> float:
        """The float cost (-ln P) of a sentence by the lookup rule, <s> implied and </s> added (khg_lm_score)."""
        w = _lib.as_np(list(words), np.int32)
        out = _lib.C.c_float(0.0)
        _lib.check(_lib.lib.khg_lm_score(*self._c_args(), int(w.shape[0]), _lib.ptr(w, _lib.C.c_int32), _lib.C.byref(out)))
        return float(out.value)

    @staticmethod
    def unigram(word_probs: Dict[int, float]) -> "NgramLm":
        """The one-state LM of TrainingGraphCompiler.compile_word_loop_graph(word_probs): cost -ln p per word, the sentence end free.
        Rescoring with it at scale -1 takes the graph's unigram out of the lattices."""
        words = sorted(int(w) for w in word_probs)
        cost = [np.float32(-math.log(float(word_probs[w]))) for w in words]
        return NgramLm([-1], [0.0], [0, len(words)], words, cost, [0] * len(words), [0.0], 0)

    @staticmethod
    def from_arpa(text: str, word2id: Dict[str, int], bos: str = "<s>", eos: str = "</s>") -> "NgramLm":
        """An ARPA backoff LM as the automaton.  States: the empty history, then every listed n-gram of order 1 .. N - 1 that does not
        end in `eos`, numbered by order, then by word-id tuple (`bos` sorts first).  A listed (h, w), w != eos, is an arc of h to the
        longest suffix of hw that is a state; cost = float(-ln(10) * log10 p), formed in double; backoff_cost likewise from the backoff
        weight (0 when absent); final_cost[h] from the `eos` entries by the lookup rule."""
        grams, header = _parse_arpa(text)
        order = max(grams) if grams else 0
        if order < 1:
            raise KhgError("NgramLm.from_arpa: no n-grams")
        for k, cnt in header.items():
            if len(grams.get(k, [])) != cnt:
                raise KhgError("NgramLm.from_arpa: the \\data\\ header announces %d %d-grams, the section lists %d" % (cnt, k, len(grams.get(k, []))))
        for k in grams:
            if k not in header:
                raise KhgError("NgramLm.from_arpa: the \\data\\ header announces no %d-grams, the section lists %d" % (k, len(grams[k])))

        def wid(tok):
            if tok == bos:
                return _BOS
            if tok == eos:
                return -1
            if tok not in word2id:
                raise KhgError("NgramLm.from_arpa: word %r is not in word2id" % tok)
            i = int(word2id[tok])
            if i <= 0:
                raise KhgError("NgramLm.from_arpa: word %r has id %d; word-ids are > 0" % (tok, i))
            return i

        entries = {}        # n-gram tuple -> (log10 p, backoff weight)
        for k in sorted(grams):
            for logp, toks, bow in grams[k]:
                entries[tuple(wid(t) for t in toks)] = (logp, bow)
        if (-1,) not in entries:
            raise KhgError("NgramLm.from_arpa: no unigram for %s" % eos)
        if (_BOS,) not in entries:
            raise KhgError("NgramLm.from_arpa: no unigram for %s" % bos)
        hists = sorted((g for g in entries if len(g) < order and g[-1] != -1), key=lambda g: (len(g), g))
        state = {(): 0}
        for g in hists:
            state[g] = len(state)

        def longest_suffix(g):
            while g not in state:
                g = g[1:]
            return state[g]

        ln10 = math.log(10.0)
        n = len(state)
        backoff = np.full(n, -1, np.int32)
        backoff_cost = np.zeros(n, np.float32)
        for g, h in state.items():
            if h:
                backoff[h] = longest_suffix(g[1:])
                backoff_cost[h] = np.float32(-ln10 * entries[g][1])
        arcs = [[] for _ in range(n)]
        eos_cost = {}
        for g, (logp, _) in entries.items():
            h, w = g[:-1], g[-1]
            if h not in state:
                raise KhgError("NgramLm.from_arpa: the history of the %d-gram %r is not listed" % (len(g), g))
            if w == -1:
                eos_cost[state[h]] = np.float32(-ln10 * logp)
            elif w != _BOS:
                arcs[state[h]].append((w, np.float32(-ln10 * logp), longest_suffix(g if len(g) < order else g[1:])))
        final = np.zeros(n, np.float32)
        for h in range(n):
            c, x = np.float32(0.0), h
            while x not in eos_cost:
                c = np.float32(c + backoff_cost[x])
                x = int(backoff[x])
            final[h] = np.float32(c + eos_cost[x])
        return _from_arc_lists(backoff, backoff_cost, arcs, final, state[(_BOS,)])


def _from_arc_lists(backoff, backoff_cost, arcs, final, start) -> NgramLm:
    arc_begin = np.zeros(len(arcs) + 1, np.int32)
    word, cost, nxt = [], [], []
    for h, lst in enumerate(arcs):
        lst = sorted(lst)
        word += [a[0] for a in lst]
        cost += [a[1] for a in lst]
        nxt += [a[2] for a in lst]
        arc_begin[h + 1] = len(word)
    return NgramLm(backoff, backoff_cost, arc_begin, word, cost, nxt, final, start)


def _parse_arpa(text: str):
    """-> ({order: [(log10 p, tokens, backoff weight)]}, {order: announced count})"""
    grams: Dict[int, List[Tuple[float, List[str], float]]] = {}
    header: Dict[int, int] = {}
    sec = None
    for raw in text.splitlines():
        line = raw.strip()
        if not line:
            continue
        if line == "\\data\\":
            sec = 0
        elif line == "\\end\\":
            break
        elif line.startswith("\\") and line.endswith("-grams:"):
            sec = int(line[1:-len("-grams:")])
            grams.setdefault(sec, [])
        elif sec == 0 and line.startswith("ngram"):
            k, cnt = line[len("ngram"):].split("=")
            header[int(k)] = int(cnt)
        elif sec:
            f = line.split()
            if len(f) not in (sec + 1, sec + 2):
                raise KhgError("NgramLm.from_arpa: a %d-gram line has %d fields: %r" % (sec, len(f), line))
            grams[sec].append((float(f[0]), f[1:sec + 1], float(f[sec + 1]) if len(f) == sec + 2 else 0.0))
    return grams, header


def estimate_ngram_lm(transcripts: Iterable[Sequence[int]], order: int, vocab: Iterable[int], discount: float = 0.5) -> NgramLm:
    """A small interpolated absolute-discounting estimator in backoff form.  transcripts: word-id sequences; vocab: the word-ids (> 0)
    the LM knows.  For a history h seen c(h) times before t(h) distinct words (the sentence end among them):
        P(w | h) = max(c(h, w) - D, 0) / c(h) + D t(h) / c(h) * P(w | h without its first word)
    and below the empty history the uniform distribution over the vocabulary and the sentence end.  A listed (h, w) is an arc with that
    probability; a word h does not list backs off with weight D t(h) / c(h), which is what the formula gives.  So for every history the
    probabilities of the vocabulary and the sentence end sum to 1 through the backoff rule."""
    vocab = sorted(set(int(w) for w in vocab))
    if order < 1 or not vocab or vocab[0] <= 0 or not 0.0 < discount < 1.0:
        raise KhgError("estimate_ngram_lm: order >= 1, a vocabulary of word-ids > 0 and 0 < discount < 1")
    EOS = -1
    counts: Dict[tuple, Dict[int, int]] = {(): {}}
    known = set(vocab)
    for t in transcripts:
        seq = [_BOS] + [int(w) for w in t] + [EOS]
        for w in seq[1:-1]:
            if w not in known:
                raise KhgError("estimate_ngram_lm: word %d is not in the vocabulary" % w)
        for i in range(1, len(seq)):
            for m in range(0, min(order - 1, i) + 1):
                d = counts.setdefault(tuple(seq[i - m:i]), {})
                d[seq[i]] = d.get(seq[i], 0) + 1
    hists = sorted((h for h in counts if h), key=lambda g: (len(g), g))
    state = {(): 0}
    for h in hists:
        state[h] = len(state)
    uniform = 1.0 / (len(vocab) + 1)
    prob: Dict[tuple, Dict[int, float]] = {}
    gamma: Dict[tuple, float] = {}

    def p(h, w):      # the backoff rule, in double
        return prob[h][w] if w in prob[h] else gamma[h] * p(h[1:], w)

    for h in [()] + hists:
        c = counts[h]
        tot = sum(c.values())
        gamma[h] = discount * len(c) / tot if tot else 1.0
        if h:
            prob[h] = {w: (k - discount) / tot + gamma[h] * p(h[1:], w) for w, k in c.items()}
        else:
            prob[h] = {w: (max(c.get(w, 0) - discount, 0.0) / tot if tot else 0.0) + gamma[h] * uniform for w in vocab + [EOS]}

    def longest_suffix(g):
        while g not in state:
            g = g[1:]
        return state[g]

    n = len(state)
    backoff = np.full(n, -1, np.int32)
    backoff_cost = np.zeros(n, np.float32)
    final = np.zeros(n, np.float32)
    arcs = [[] for _ in range(n)]
    for h, s in state.items():
        if s:
            backoff[s] = state[h[1:]]
            backoff_cost[s] = np.float32(-math.log(gamma[h]))
        final[s] = np.float32(-math.log(p(h, EOS)))
        for w, q in prob[h].items():
            if w != EOS:
                g = h + (w,)
                arcs[s].append((w, np.float32(-math.log(q)), longest_suffix(g if len(g) < order else g[1:])))
    return _from_arc_lists(backoff, backoff_cost, arcs, final, state.get((_BOS,), 0))
