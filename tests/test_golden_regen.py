"""The golden fixtures are what the committed generators produce: tests/golden/check_fixtures.py regenerates every one from the
reference checkout and compares the files byte for byte.  Run as a child process: the generators stub sys.modules, patch torch's
random sources and set its thread count, and ref_harness sets process-wide state on import."""
import os
import subprocess
import sys

import pytest

SCRIPT = os.path.join(os.path.dirname(__file__), "golden", "check_fixtures.py")
NO_REFERENCE = 3          # check_fixtures.py's exit status where the reference checkout is absent


def test_generators_reproduce_committed_fixtures():
    p = subprocess.run([sys.executable, SCRIPT], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode == NO_REFERENCE:
        pytest.skip(p.stdout.strip())
    assert p.returncode == 0, p.stdout
