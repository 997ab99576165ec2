"""The post-training batch check (kelpie_amd/csrc/kp_batch_check.hpp) under the host sanitizers.

Every ``*_posttrain_rank`` of the library runs ``kp_check_batch`` before its first upload
or launch.  ``make batch_asan`` builds the header alone into
``tests/native/batch_check_driver.cpp`` with ``-fsanitize=address,undefined``; the driver
checks one well-formed batch of 3 slots (with ``n_ent`` as head, tail, ranked object and
filter id) and, for every rule, that batch with exactly that rule broken (``n_ent + 1``
and ``-1`` as ids, ``n_rel2`` as a relation, offsets that decrease, a ranked triple that
does not start at the kelpie entity).  The good batch must pass, every bad one must yield a
message, and neither sanitizer may report.  Malformed batches never reach a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def test_batch_check_under_asan():
    r = subprocess.run(["make", "-C", ROOT, "batch_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([os.path.join(ROOT, "build", "san", "batch_check_asan")], capture_output=True, text=True,
                       env=env, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    for marker in ("AddressSanitizer", "LeakSanitizer", "runtime error"):
        assert marker not in p.stderr, p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[0] == "good: ok" and lines[1] == "empty: ok", p.stdout
    assert lines[-1].endswith(" 0 failures"), p.stdout
    assert len(lines) >= 2 + 12 + 1 and "ACCEPTED" not in p.stdout, p.stdout
