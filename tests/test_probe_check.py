"""The probes' host check and chunking (kelpie_amd/csrc/kp_probe_check.hpp), plain and under
the host sanitizers.

``make probe_check probe_check_asan`` builds the header alone into
``tests/native/probe_check_driver.cpp``, once plain and once with
``-fsanitize=address,undefined``.  The driver passes a good set of probes (an empty slot
between full ones; no probes at all with null arrays), breaks each rule of the check once in
the good set and requires that rule's message, expands the good set into rank rows (the
empty slot between two that have probes) and a batch's slots likewise (0, 1 and 3 slots, the
kelpie entity among the objects), and on 400 pseudo-random valid sets requires
that the check passes and that the chunks cover every probe row once, in whole groups of 16
rows, within their budget (or as KP_PROBE_CHUNK forces them).  No kernel runs: malformed
probes never reach a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

MESSAGES = ("probe_off must start at 0", "probe_off decreases", "probe_off must end at the probe count",
            "negative probe count", "missing probe_off", "missing probes", "missing filt_off", "missing filt",
            "missing probe output", "probe relation out of range", "probe object out of range",
            "filt_off must start at 0", "filt_off decreases", "probe filter id out of range", "empty model",
            "negative n_slots")


@pytest.mark.parametrize("target", ["probe_check", "probe_check_asan"])
def test_probe_check(target):
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
    assert "random sets: 400" in lines, p.stdout
    assert "good: ok" in lines and "no probes, null arrays: ok" in lines, p.stdout
    assert "rows, empty middle slot: ok" in lines and "rows, no probes: ok" in lines, p.stdout
    for n in ("no slots", "one slot", "three slots"):
        assert f"slot rows, {n}: ok" in lines, p.stdout
    # every rule was broken at least once and reported
    told = [ln.split(": ", 1)[1] for ln in lines if ": " in ln]
    assert all(m in told for m in MESSAGES), p.stdout
