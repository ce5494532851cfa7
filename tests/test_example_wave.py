"""examples/train_wave_synthetic.py end to end: synthetic YES/NO waveforms, MFCC on the device, per-utterance
CMVN and deltas on the device, ML training of the monophone model, decoding of held-out utterances.  The example exits 0: the
held-out WER is at most its --max-wer.  The example's defaults: the flat-start recipe needs its full schedule."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs_and_decodes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_wave_synthetic.py")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    m = re.search(r"RESULT wer=(\S+) like=(\S+)", r.stdout)
    assert m, "no RESULT line"
    assert float(m.group(1)) <= 0.2
