"""The rank margins' host check and threshold rule (kelpie_amd/csrc/kp_margins_check.hpp), plain
and under the host sanitizers.

``make margins margins_asan`` builds the header alone into ``tests/native/margins_driver.cpp``,
once plain and once with ``-fsanitize=address,undefined``.  The driver passes good requests,
breaks each rule of the check once and requires that rule's message and code, and holds the
threshold rule against hand-computed values: ``tol`` = 0 gives the target's value itself (also
where the square of its rounded root is another double), the L2 lower threshold is clamped at
0, a swallowed L2 delta never carries a threshold across the target, and on 2,000 pseudo-random
rows the thresholds bracket the target and nest with ``tol``.  No kernel runs: a malformed
request never reaches a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

# each rule of the check, by the cases that break it alone
RULES = (("null request", "missing request"), ("nan tol", "tol is NaN"), ("negative tol", "negative tol"),
         ("tol above 1", "tol above 1"), ("infinite tol", "tol above 1"),
         ("slots: rank_lo alone", "rank_lo and rank_hi go together"),
         ("probes: rank_hi alone", "rank_lo and rank_hi go together"),
         ("marks: rank_lo alone", "rank_lo and rank_hi go together"),
         ("probe outputs, no probes", "probe outputs without probes"),
         ("one probe output, no probes", "probe outputs without probes"),
         ("mark outputs, no marks", "mark outputs without marks"),
         ("fp32 rank", "margins need the fp64 rank (the fp32 rank switch is set)"),
         ("fp32 rank, bad tol", "tol above 1"))
GOOD = ("good", "good: slots alone", "good: tol 0", "good: tol 1", "good: ties alone")
THRESHOLDS = ("dot 0.5 lo", "dot 0.5 hi", "logit -4 lo", "logit -4 hi", "l1 8 lo", "l1 8 hi", "l2 16 lo", "l2 16 hi",
              "l2 clamp lo", "l2 clamp hi", "l2 zero distance lo", "l2 zero distance hi", "units l2", "units l1",
              "tol 0 negative score lo")


@pytest.mark.parametrize("target", ["margins", "margins_asan"])
def test_margins_check(target):
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
    assert "random rows: 2000" in lines and "l2 tiny tol: checked" in lines, p.stdout
    for case in GOOD + THRESHOLDS:
        assert f"{case}: ok" in lines, (case, p.stdout)
    for case, msg in RULES:
        assert f"{case}: {msg}" in lines, (case, p.stdout)
    # tol == 0 gives c_t itself: four kinds, four values, both thresholds
    assert sum(ln.startswith("tol 0 mode ") and ln.endswith(": ok") for ln in lines) == 32, p.stdout
