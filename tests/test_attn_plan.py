"""The attention planners (kelpie_amd/csrc/kp_attn_plan.hpp), plain and under the host sanitizers.

``make attn_plan attn_plan_asan`` builds the header alone into
``tests/native/attn_plan_driver.cpp``, once plain and once with
``-fsanitize=address,undefined``.  For nq in {1, 63, 64, 65, 1029, 4204, 20000}, n_ent in
{33, 517, 14541}, slots in {8, 256, 512} and the in-flight hint in {1, 2, 3, 4} the driver
checks what ``kp_attn3`` and the merge kernels rely on: 1 <= S <= min(16, ktq),
``n_parts == S``, ``n_wg >= 8`` and a multiple of 8, key ranges that tile [0, ktq) with
none empty, and -- replaying the kernel's own unit walk -- every (query tile, range) unit
visited exactly once.  Hint 1 must give the plan of a launch that runs alone, unchanged
(3000 -> (5, 240), 3730 -> (13, 256), 4204 -> (11, 256), 4500 -> (7, 256) at 256 slots and
14541 entities); a hint >= 2 one workgroup per unit, ``n_wg == ceil8(QT * S)``.  No kernel
runs: a bad plan never reaches a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.mark.parametrize("target", ["attn_plan", "attn_plan_asan"])
def test_attn_plans(target):
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
    assert lines[0].startswith("grid: ") and int(lines[0].split()[1]) >= 7 * 3 * 3 * 4, p.stdout
    assert lines[-1] == "0 failures" and "FAIL" not in p.stdout, p.stdout
