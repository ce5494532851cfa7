"""examples/score_lattices_synthetic.py end to end at its smallest size: one lattice-faster decode of the YES/NO
task on the shared word loop, the sweep of score.sh over 33 (LMWT, penalty) points in one call, the oracle.  The example exits 0 only
if the point it also scores the old way (best_path, the words on the host, compute_wer) and every host oracle agree with the device.
The oracle path is one of the lattice's paths and every point of the sweep scores one of them, so the best WER of the table cannot be
below the oracle WER."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs_and_its_best_wer_is_not_below_its_oracle_wer():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "score_lattices_synthetic.py"), "--utts", "60", "--test-utts", "20", "--iters", "30"],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:], r.stderr[-3000:])
    assert r.returncode == 0
    m = re.search(r"RESULT best_wer=(\S+) best_lmwt=(\d+) best_penalty=(\S+) oracle_wer=(\S+) host_agrees=(\d)", r.stdout)
    assert m, "no RESULT line"
    assert m.group(5) == "1" and 7 <= int(m.group(2)) <= 17
    assert 0.0 <= float(m.group(4)) <= float(m.group(1)) <= 1.0
    assert len(re.findall(r"^LMWT +\d+ ", r.stdout, re.M)) == 11
