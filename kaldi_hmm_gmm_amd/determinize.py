"""Determinizing lattices on the device (the rule is written out at khg_lattices_determinize in include/khg_hip.h):
Kaldi's lattice-determinize-pruned, and LatticeFasterDecoder::GetLattice -- the raw lattice followed, when the configuration asks for
it, by the determinization the decoder's lattice_beam and det_opts.delta describe -- on the lattices a decode left in HBM."""
from . import _gpu


def _on_device(lattices):
    from .align import DeviceLattices
    on = isinstance(lattices, DeviceLattices)
    return on, lattices if on else DeviceLattices.from_lattices(list(lattices), _gpu.default_context())


def lattice_determinize_pruned_batch(lattices, graph_scale: float = 1.0, acoustic_scale: float = 1.0, beam: float = 10.0,
                                     delta: float = 1.0 / 1024, state_factor: int = 8, return_stats: bool = False):
    """Kaldi's lattice-determinize-pruned for several utterances on the device (khg_lattices_determinize): per utterance a lattice in
    which every word sequence of the beam-pruned input has exactly one path, the cheapest, made of copies of the input's arcs.
    lattices: a list of Lattice (-> a list of Lattice; an utterance that did not succeed is empty) or a DeviceLattices (-> a
    DeviceLattices carrying .status).  return_stats: -> (that, status [U], stats)."""
    on, dl = _on_device(lattices)
    try:
        res, status, stats = dl.determinize(float(graph_scale), float(acoustic_scale), float(beam), float(delta), int(state_factor))
    finally:
        if not on:
            dl.close()
    if not on:
        out = res.download()
        res.close()
        res = out
    return (res, status, stats) if return_stats else res


def lattice_determinize_pruned(lattice, graph_scale: float = 1.0, acoustic_scale: float = 1.0, beam: float = 10.0, delta: float = 1.0 / 1024,
                               state_factor: int = 8):
    """lattice-determinize-pruned for one utterance -> the Lattice (lattice_determinize_pruned_batch of one)"""
    return lattice_determinize_pruned_batch([lattice], graph_scale, acoustic_scale, beam, delta, state_factor)[0]


def _determinized(dl, config, state_factor):
    if not config.determinize_lattice:
        return dl
    res, _, _ = dl.determinize(1.0, 1.0, float(config.lattice_beam), float(config.det_opts.delta), int(state_factor))
    dl.close()
    return res


def get_lattice_faster_device_batch(am, tm, fsts, feats_list, config, acoustic_scale, allow_partial=True, scratch_per_frame=0,
                                    return_scores=False, state_factor: int = 8):
    """LatticeFasterDecoder::GetLattice for a batch, the lattices staying on the device: get_raw_lattice_faster_device_batch followed,
    when config.determinize_lattice is set, by determinize(1, 1, config.lattice_beam, config.det_opts.delta).  -> (the decode's dicts,
    DeviceLattices)"""
    from .align import get_raw_lattice_faster_device_batch
    res, dl = get_raw_lattice_faster_device_batch(am, tm, fsts, feats_list, config, acoustic_scale, allow_partial, scratch_per_frame, return_scores)
    return res, _determinized(dl, config, state_factor)


def get_lattice_faster_batch(am, tm, fsts, feats_list, config, acoustic_scale, allow_partial=True, scratch_per_frame=0, return_scores=False,
                             state_factor: int = 8):
    """The same with the lattices downloaded: the decode's dicts, each with its "lattice" (empty where the decode or the determinization
    did not succeed)"""
    res, dl = get_lattice_faster_device_batch(am, tm, fsts, feats_list, config, acoustic_scale, allow_partial, scratch_per_frame, return_scores,
                                              state_factor)
    for d, lat in zip(res, dl.download()):
        d["lattice"] = lat
    dl.close()
    return res
