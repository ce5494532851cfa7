"""examples/nbest_synthetic.py end to end at its smallest size: one lattice-faster decode of the YES/NO task on
the shared word loop, determinize, the 10-best lists of the lattices left on the device, every entry rescored on the host with a
bigram.  The example exits 0 only if the host form equals the device on every list and the word sequences of every list are pairwise
distinct.  The 1-best is an entry of its list, so the WER of the best entry of each list must be <= the 1-best's."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs_and_the_oracle_of_the_list_is_no_worse():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "nbest_synthetic.py"), "--utts", "60", "--test-utts", "20", "--iters", "30"],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:], r.stderr[-3000:])
    assert r.returncode == 0
    m = re.search(r"RESULT wer_best=([\d.]+) wer_rescored=([\d.]+) wer_oracle=([\d.]+) entries=(\d+) failed=(\d+) distinct=(\d) host_agrees=(\d)", r.stdout)
    assert m, "no RESULT line"
    assert m.group(6) == "1" and m.group(7) == "1" and int(m.group(5)) < 20
    assert float(m.group(3)) <= float(m.group(1))
    assert int(m.group(4)) > 20 - int(m.group(5))          # some list has more than one entry
    assert re.search(r"^WER of the 1-best", r.stdout, re.M)
