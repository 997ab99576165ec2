"""The attributions' host check and the step plan's row map (kelpie_amd/csrc/kp_attrib_check.hpp,
kelpie_amd/csrc/kp_cx_rowmap.hpp), plain and under the host sanitizers.

``make attrib attrib_asan`` builds the two headers alone into ``tests/native/attrib_driver.cpp``,
once plain and once with ``-fsanitize=address,undefined``.  The driver passes good requests,
breaks each rule of the check once and requires that rule's message and code (and, with two rules
broken, the earlier one), holds the row map of two hand-written batches against hand-derived
maps (a repeated relation and pair, a self-loop, a duplicate row, an empty slot; a multi-step
slot's permuted minibatches) and checks the map's index invariants on 200 pseudo-random batches.
No kernel runs: a malformed request never reaches a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

LINEAR = "attributions serve ComplEx and DistMult only (the score must be linear in the row)"
ADAM = "attributions are not offered with Adam (Adagrad and SGD only)"
QUAD = "the tail of a slot's pred is the kelpie entity (its score is quadratic in the row)"
# each rule of the check, by the cases that break it
RULES = (("null request", "missing request"), ("null out_fit", "missing out_fit or out_reg"),
         ("null out_reg", "missing out_fit or out_reg"), ("null out_delta", "missing out_delta"),
         ("TransE", LINEAR), ("ConvE", LINEAR), ("Adam", ADAM), ("kelpie tail", QUAD),
         ("null out_fit on TransE", "missing out_fit or out_reg"), ("TransE with Adam", LINEAR),
         ("Adam with a kelpie tail", ADAM))
GOOD = ("good: ComplEx Adagrad", "good: DistMult", "good: SGD", "good: no rows, delta alone", "good: no slots")
MAPS = tuple(f"hand {kind}: {what}" for kind, names in
             (("single-step", ("map", "targets", "tg_row", "qk_off", "qk_row", "t_off", "t_row")),
              ("multi-step", ("map", "tg_row", "qk_off", "qk_row", "t_off", "t_row"))) for what in names)


@pytest.mark.parametrize("target", ["attrib", "attrib_asan"])
def test_attrib_check(target):
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
    assert "random batches: 200" in lines and "random rows: many" in lines, p.stdout
    assert "hand multi-step: another batch_size: refused" in lines, p.stdout
    for case in GOOD + MAPS:
        assert f"{case}: ok" in lines, (case, p.stdout)
    for case, msg in RULES:
        assert f"{case}: {msg}" in lines, (case, p.stdout)
