"""The post-training step planners (kelpie_amd/csrc/kp_cx_plan.hpp: ComplEx / DistMult,
kp_cv_plan.hpp: ConvE), plain and under the host sanitizers.

``make step_plan step_plan_asan`` builds the two headers alone into
``tests/native/step_plan_driver.cpp``, once plain and once with
``-fsanitize=address,undefined``.  The driver compares every array of the plan of a few tiny
batches (one step, several steps, mixed slots, no epochs; ConvE tail dedup with one and with
three dropouts, shared-encoder rows and frozen chunks) with values derived by hand from the
rules; breaks each of the planners' five rules once in a good batch and requires that rule's
message (permutation values R and -1, a ``rng_off`` that decreases across a slot); and on 400
pseudo-random batches (up to 8 slots of up to 40 rows, batch_size 1..8) checks what the
kernels rely on when they index with the plan: offset vectors non-decreasing and ending at
their list's size, every stored index inside the array it indexes, every row accounted for
once per plan, and each ConvE step's instances equal to that batch's pairs.  No kernel runs:
a bad plan never reaches a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

MESSAGES = ("a training row does not involve the kelpie entity", "missing randperm draws for a multi-step slot",
            "randperm value out of range", "missing dropout keep bits")


@pytest.mark.parametrize("target", ["step_plan", "step_plan_asan"])
def test_step_plans(target):
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
    # every rule was broken at least once (the first message by both planners) and reported
    told = [ln.split(": ", 1)[1] for ln in lines if ": " in ln]
    assert told.count(MESSAGES[0]) >= 3 and all(m in told for m in MESSAGES), p.stdout
