"""The epoch marks' host check and mark plan (kelpie_amd/csrc/kp_marks_check.hpp), plain and
under the host sanitizers.

``make marks_check marks_check_asan`` builds the header alone into
``tests/native/marks_check_driver.cpp``, once plain and once with
``-fsanitize=address,undefined``.  The driver passes a good request, breaks each rule of the
check once and requires that rule's message, compares the plan with hand-derived ones (slots
of 1, 2 and 3 steps per epoch and an empty slot in one batch, the marks {0}, {E} and all of
0..15, ConvE's pair counts with a last step of one pair) and, on 400 pseudo-random batches,
with a second statement of the rule; it expands two slots by two marks into rank rows (one
slot's filter list empty) and requires that 2^31 and 2^32 filter entries, reached by the
offsets alone, are refused.  No kernel runs: a malformed request never reaches a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

MESSAGES = ("missing epochs", "n must be in [1, 16]", "epochs must be strictly increasing", "negative epoch",
            "epoch beyond hp->epochs", "missing mark output", "missing hyper-parameters", "negative epochs",
            "unknown model", "batch_size must be positive")
PLANS = ("rows model 0 3/0/2/1 steps", "rows model 1 3/0/2/1 steps", "rows model 3 3/0/2/1 steps", "mark {0}",
         "mark {E}", "no epoch", "pairs bs 3", "pairs bs 2", "marks 0..15")


@pytest.mark.parametrize("target", ["marks_check", "marks_check_asan"])
def test_marks_check(target):
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
    assert "random batches: 400" in lines and "good: ok" in lines, p.stdout
    for plan in PLANS:
        assert f"{plan}: ok" in lines, (plan, p.stdout)
    for rows in ("rows 2 x 2, one empty filter", "rows without a filter"):
        assert f"{rows}: ok" in lines, (rows, p.stdout)
    for case in ("rows: 2^31 filter entries", "rows: 2^32 filter entries"):
        assert f"{case}: the mark rows' filter lists exceed 2^31 - 1 entries" in lines, (case, p.stdout)
    assert "rows: too many: too many mark rows" in lines, p.stdout
    # every rule was broken at least once and reported
    told = [ln.rsplit(": ", 1)[1] for ln in lines if ": " in ln]
    assert all(m in told for m in MESSAGES), p.stdout
    # each of the six rules of the check, by the case that breaks it alone
    for case, msg in (("null epochs", "missing epochs"), ("n 0", "n must be in [1, 16]"),
                      ("n 17", "n must be in [1, 16]"), ("repeated", "epochs must be strictly increasing"),
                      ("negative", "negative epoch"), ("beyond", "epoch beyond hp->epochs"),
                      ("null out_rank", "missing mark output")):
        assert f"{case}: {msg}" in lines, (case, p.stdout)
