"""The post-training trace's step counts and host check (kelpie_amd/csrc/kp_trace_check.hpp),
plain and under the host sanitizers.

``make trace_check trace_check_asan`` builds the header alone into
``tests/native/trace_check_driver.cpp``, once plain and once with
``-fsanitize=address,undefined``.  The driver compares kp_trace_steps' rule with hand-derived
counts (every family, an empty slot, no epoch, a last step of one row or one pair), passes a
good trace, breaks each rule of the check once and requires that rule's message, and on 400
pseudo-random batches requires the counts of a second statement of the rule, a passing check
on their prefix sums and a failing one on every offset moved by one.  No kernel runs: a
malformed trace never reaches a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

MESSAGES = ("missing trace_off", "trace_off must start at 0", "trace_off disagrees with kp_trace_steps",
            "missing out_loss", "batch_size must be positive", "negative epochs", "missing hyper-parameters",
            "unknown model", "negative n_slots", "missing row_off", "missing rows", "row_off must start at 0",
            "row_off decreases", "missing out_steps", "more than 2^31 - 1 steps")


@pytest.mark.parametrize("target", ["trace_check", "trace_check_asan"])
def test_trace_check(target):
    r = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([os.path.join(ROOT, "build", "san", target)], capture_output=True, text=True, env=env,
                       timeout=120)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    for marker in ("AddressSanitizer", "LeakSanitizer", "runtime error"):
        assert marker not in p.stderr, p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "0 failures" and "FAIL" not in p.stdout, p.stdout
    assert "random batches: 400" in lines, p.stdout
    assert "good: ok" in lines and "no step, null out_loss: ok" in lines and "no slots: ok" in lines, p.stdout
    assert "pairs bs 3: ok" in lines and "rows model 1 bs 6: ok" in lines, p.stdout
    # every rule was broken at least once and reported
    told = [ln.split(": ", 1)[1] for ln in lines if ": " in ln]
    assert all(m in told for m in MESSAGES), p.stdout
