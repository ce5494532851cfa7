"""examples/train_cmvn_deltas_synthetic.py end to end: static features under a per-speaker offset and gain, the
model's features made on the device as add-deltas of the raw rows and as apply-cmvn | add-deltas with per-speaker statistics, ML
training on each in the same schedule, decoding of held-out speakers both ways.  The example exits 0 and the normalised features
decode no worse.  The example's defaults: the flat-start recipe needs its full schedule (examples/decode_synthetic.py says why)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs_and_cmvn_does_not_hurt():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_cmvn_deltas_synthetic.py")], capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    m = re.search(r"RESULT wer_raw=(\S+) wer_cmvn=(\S+) like_raw=(\S+) like_cmvn=(\S+)", r.stdout)
    assert m, "no RESULT line"
    wer_raw, wer_cmvn, like_raw, like_cmvn = map(float, m.groups())
    assert wer_cmvn <= wer_raw
