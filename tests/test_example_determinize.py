"""examples/determinize_synthetic.py end to end at its smallest size: one lattice-faster decode of the YES/NO task
on the shared word loop, then lattice-determinize-pruned of the lattices it left on the device, and lm_rescore and MBR on both.  The
example exits 0 only if the host form equals the device on every lattice, get_lattice_faster_device_batch gives the same lattices, and
the best path of every determinized lattice is the raw lattice's in words and weight.  The WERs are printed, not asserted."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs_and_host_and_device_agree():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "determinize_synthetic.py"), "--utts", "60", "--test-utts", "20", "--iters", "30"],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:], r.stderr[-3000:])
    assert r.returncode == 0
    m = re.search(r"RESULT states_raw=(\d+) states_det=(\d+) lm_states_raw=(\d+) lm_states_det=(\d+) failed=(\d+) host_agrees=(\d)", r.stdout)
    assert m, "no RESULT line"
    assert m.group(6) == "1" and int(m.group(5)) < 20
    assert 0 < int(m.group(1)) and 0 < int(m.group(2)) and 0 < int(m.group(3)) and 0 < int(m.group(4))
    assert re.search(r"^determinized: \d+ states", r.stdout, re.M) and re.search(r"^  det: bigram lm_rescore", r.stdout, re.M)
