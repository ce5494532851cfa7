"""examples/mbr_decode_synthetic.py end to end at its smallest size: one lattice-faster decode of the YES/NO task
on the shared word loop, then minimum Bayes risk decoding and word confidences of the lattices it left on the device.  The example
exits 0 only if every position's gammas sum to 1 within the bound of mass conservation -- (states + arcs) * (Q + 1) * 2^-52 -- and the
host form, given the device's weights, equals the device on every output.  The WERs are printed, not asserted: MBR minimises the
EXPECTED error under the model, which on 20 utterances need not be the realised one."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_example_runs_and_every_bin_sums_to_one():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "mbr_decode_synthetic.py"), "--utts", "60", "--test-utts", "20", "--iters", "30"],
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-4000:], r.stderr[-3000:])
    assert r.returncode == 0
    m = re.search(r"RESULT map_wer=(\S+) mbr_wer=(\S+) gamma_sum_over_bound=(\S+) failed=(\d+) host_agrees=(\d)", r.stdout)
    assert m, "no RESULT line"
    assert m.group(5) == "1" and 0.0 <= float(m.group(3)) <= 1.0 and int(m.group(4)) < 20
    assert 0.0 <= float(m.group(1)) and 0.0 <= float(m.group(2))
    assert re.search(r"^MAP WER \S+%   MBR WER \S+%", r.stdout, re.M) and re.search(r"^mean confidence: ", r.stdout, re.M)
