"""examples/train_tri_synthetic.py end to end at its smallest size: mono training, acc-tree-stats on the device,
build-tree, gmm-init-model, convert-ali, training and decoding on triphone graphs.  Every transcript compiles and aligns on the tri
graphs; the tree has more pdfs than the monophone system and at most max_leaves; objf_impr is positive and equals the sum of the leaves'
Objf minus the sum of the stub leaves' Objf, recomputed here from the downloaded statistics, to 1e-9 relative (no leaves are merged:
--cluster-thresh 0).  The WER is printed, not asserted."""
import os
import pickle
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tree_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_builds_and_trains_a_triphone_system(tmp_path):
    out = str(tmp_path / "tree.pkl")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_tri_synthetic.py"), "--utts", "40", "--test-utts", "10", "--iters", "10",
                        "--max-leaves", "30", "--cluster-thresh", "0", "--out", out], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    m = re.search(r"RESULT failed_compile=(\d+) failed_align=(\d+) mono_pdfs=(\d+) tri_pdfs=(\d+) max_leaves=(\d+) objf_impr=(\S+)", r.stdout)
    assert m, "no RESULT line"
    failed_compile, failed_align, mono_pdfs, tri_pdfs, max_leaves = (int(m.group(i)) for i in range(1, 6))
    assert failed_compile == 0 and failed_align == 0
    assert mono_pdfs < tri_pdfs <= max_leaves
    with open(out, "rb") as fh:
        d = pickle.load(fh)
    impr = d["info"]["objf_impr"]
    assert impr > 0 and float(m.group(6)) == impr and d["info"]["num_removed"] == 0
    st, tree = d["stats"], d["tree"]
    dim = st["x"].shape[1]
    leaves, stubs = {}, {}
    for i, key in enumerate(st["keys"].tolist()):
        if key[1] == 1:
            continue                                   # silence: its root is not split, leaf and stub leaf are the same
        ok, pdf = tree.compute(key[:3], key[3])
        assert ok
        for table, k in ((leaves, pdf), (stubs, key[1])):          # shared roots of one phone each: the stub leaf is the central phone
            table.setdefault(k, ref.Gauss(dim)).add(float(st["count"][i]), st["x"][i].tolist(), st["x2"][i].tolist())
    want = sum(g.objf(0.01) for g in leaves.values()) - sum(g.objf(0.01) for g in stubs.values())
    print("objf_impr", impr, "recomputed", want)
    assert abs(impr - want) <= 1e-9 * abs(want)
