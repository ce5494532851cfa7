"""examples/train_lda_mllt_synthetic.py end to end: ML training on noisy single frames, LDA on +-4 spliced
frames from the alignment (silence weight 0), a model on the projected rows from the same alignment, MLLT on top, decoding through the
composed final.mat.  The example exits 0; every held-out utterance decodes; the WER after is not worse than before; the kept
eigenvalues descend and the first is positive.  The example's defaults, as tests/test_example_mllt.py."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs_and_context_does_not_hurt():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_lda_mllt_synthetic.py")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    m = re.search(r"RESULT wer_before=(\S+) wer_after=(\S+) failed=(\d+) eig=(\S+)", r.stdout)
    assert m, "no RESULT line"
    wer_before, wer_after, failed = float(m.group(1)), float(m.group(2)), int(m.group(3))
    eig = [float(v) for v in m.group(4).split(",")]
    assert failed == 0 and wer_after <= wer_before
    assert eig[0] > 0 and all(a >= b for a, b in zip(eig, eig[1:]))
