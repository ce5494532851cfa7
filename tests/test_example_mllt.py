"""examples/train_mllt_synthetic.py end to end: ML training on features mixed by a fixed matrix, MLLT from the
alignment, transform-feats and gmm-transform-means, more ML iterations, decoding.  The example exits 0; the per-frame likelihood
(with log |det M|) after is above the one before; the WER is not worse.  The example's defaults: the flat-start recipe needs its full
schedule (examples/decode_synthetic.py says why), and the whole run takes a few seconds."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs_and_mllt_helps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_mllt_synthetic.py")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    m = re.search(r"RESULT like_before=(\S+) like_after=(\S+) wer_before=(\S+) wer_after=(\S+)", r.stdout)
    assert m, "no RESULT line"
    like_before, like_after, wer_before, wer_after = map(float, m.groups())
    assert like_after > like_before
    assert wer_after <= wer_before
