"""N-best lists of lattices on the device (the rule is written out at khg_lattices_nbest in include/khg_hip.h):
Kaldi's lattice-to-nbest | nbest-to-linear.  DeviceLattices.nbest(n) leaves the n cheapest paths of every utterance on the device as a
DeviceNbest; its download() gives the flat arrays, NbestList wraps them with per-utterance views.  After determinize every word sequence
has one path, so lattice_to_nbest (determinize=True, the default) lists the n best distinct word sequences."""
from . import _gpu
from ._kaldi_hmm_gmm_amd import DeviceNbest  # noqa: F401

KHG_NBEST_MAX = 1024


class NbestList:
    """The downloaded n-best lists of a batch: status [U], entry_off [U + 1], and per entry words (words_off), ali (ali_off: one
    transition-id per frame of the utterance), weight [entries][2] (graph, acoustic) and total.  The accessors return views, no copies."""

    def __init__(self, arrays):
        self.status = arrays["status"]
        self.entry_off = arrays["entry_off"]
        self.words_flat, self.words_off = arrays["words"], arrays["words_off"]
        self.ali_flat, self.ali_off = arrays["ali"], arrays["ali_off"]
        self.weight, self.total = arrays["weight"], arrays["total"]

    @property
    def num_utts(self):
        return len(self.entry_off) - 1

    @property
    def counts(self):
        return self.entry_off[1:] - self.entry_off[:-1]

    def count(self, u):
        return int(self.entry_off[u + 1] - self.entry_off[u])

    def _entry(self, u, k):
        if not 0 <= k < self.count(u):
            raise IndexError("NbestList: utterance %d has %d entries" % (u, self.count(u)))
        return int(self.entry_off[u]) + k

    def words(self, u, k):
        e = self._entry(u, k)
        return self.words_flat[self.words_off[e]: self.words_off[e + 1]]

    def alignment(self, u, k):
        e = self._entry(u, k)
        return self.ali_flat[self.ali_off[e]: self.ali_off[e + 1]]

    def weights(self, u):
        """[count(u)][2]: (graph, acoustic) of every entry of utterance u"""
        return self.weight[self.entry_off[u]: self.entry_off[u + 1]]

    def totals(self, u):
        return self.total[self.entry_off[u]: self.entry_off[u + 1]]

    def entries(self, u):
        """utterance u as Lattice.nbest gives it: [(words, alignment, (graph, acoustic), total)], cheapest first"""
        out = []
        for k in range(self.count(u)):
            e = int(self.entry_off[u]) + k
            out.append((self.words(u, k).tolist(), self.alignment(u, k).tolist(), (float(self.weight[e, 0]), float(self.weight[e, 1])),
                        float(self.total[e])))
        return out


def _on_device(lattices):
    from .align import DeviceLattices
    on = isinstance(lattices, DeviceLattices)
    return on, lattices if on else DeviceLattices.from_lattices(list(lattices), _gpu.default_context())


def lattice_to_nbest_batch(lattices, n: int, graph_scale: float = 1.0, acoustic_scale: float = 1.0, determinize: bool = True, beam: float = 10.0,
                           det_opts=None, state_factor: int = 8):
    """Kaldi's lattice-to-nbest | nbest-to-linear for several utterances on the device -> an NbestList.  determinize=True (the default)
    runs khg_lattices_determinize first, under the same scale pair, with `beam` and det_opts.delta, so that the entries are the n best
    distinct word sequences (an utterance the determinization refuses keeps that status and has no entries); determinize=False gives
    the n best alignments of the lattices as they are.  lattices: a list of Lattice or a DeviceLattices."""
    on, dl = _on_device(lattices)
    det = nb = None
    try:
        src, st0 = dl, None
        if determinize:
            delta = 1.0 / 1024 if det_opts is None else float(det_opts.delta)
            det, st0, _ = dl.determinize(float(graph_scale), float(acoustic_scale), float(beam), delta, int(state_factor))
            src = det
        nb = src.nbest(int(n), float(graph_scale), float(acoustic_scale))
        arrays = nb.download()
    finally:
        for h in (nb, det, None if on else dl):
            if h is not None:
                h.close()
    if st0 is not None:
        status = arrays["status"].copy()
        bad = (st0 & 1) == 0
        status[bad] = st0[bad]
        arrays["status"] = status
    return NbestList(arrays)


def lattice_to_nbest(lattice, n: int, graph_scale: float = 1.0, acoustic_scale: float = 1.0, determinize: bool = True, beam: float = 10.0,
                     det_opts=None, state_factor: int = 8):
    """lattice-to-nbest for one utterance -> [(words, alignment, (graph, acoustic), total)] (lattice_to_nbest_batch of one)"""
    return lattice_to_nbest_batch([lattice], n, graph_scale, acoustic_scale, determinize, beam, det_opts, state_factor).entries(0)
