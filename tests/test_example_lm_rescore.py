"""examples/decode_lm_rescore_synthetic.py end to end at a small size: Markov-chain YES/NO transcripts, one
decode on the unigram word loop, the unigram taken out of the resident lattices and an estimated bigram put in, best paths over the
LM-weight sweep.  The example exits 0 only if every held-out hypothesis formed on the device equals the one formed on the host
(Lattice.lm_rescore twice, Lattice.best_path) at every weight and no utterance failed.  The two WERs are printed; which of them is
lower at the committed seed is recorded in DESIGN.md section 7r, next to the measured figures."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs_and_device_and_host_hypotheses_agree():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "decode_lm_rescore_synthetic.py"), "--test-utts", "40"],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0
    m = re.search(r"RESULT wer_unigram=(\S+) wer_rescored=(\S+) best_unigram=(\S+) best_rescored=(\S+) host_agrees=(\d)", r.stdout)
    assert m, "no RESULT line"
    assert m.group(5) == "1"
    assert 0.0 <= float(m.group(2)) <= 1.0 and 0.0 <= float(m.group(1)) <= 1.0
