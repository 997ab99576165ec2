"""The keyed draws' pure-host header (kelpie_amd/csrc/kp_keyed.hpp), plain and under the host
sanitizers, against the numpy restatement of the definition (tests/keyed_reference.py).

``make keyed keyed_asan`` builds the header alone into ``tests/native/keyed_driver.cpp``, once
plain and once with ``-fsanitize=address,undefined``.  The driver checks Philox4x32-10's three
known answers (the Random123 vectors), the counter layout, the word counts (the int64 bound
included) and every rule of the request check, and writes a sweep of draws: R = 0, 1, 2, 63,
64, 65, 4096, 4097; epochs 0, 1, 3; n = 1, 2, 517; d = 3, 50, 260.  The sweep must equal the
restatement: the integer streams and the uniform rows bitwise, the normal rows within 1 float32
ulp (two float64 evaluations of the same formula that differ by a few float64 ulps round to
float32 values at most one float32 ulp apart).  No kernel runs."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import keyed_reference as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")

INIT_KEY, SLOT_KEY = 0x0123456789ABCDEF, 0xFEDCBA9876543210
RS, ES, NS, DS = (0, 1, 2, 63, 64, 65, 4096, 4097), (0, 1, 3), (1, 2, 517), (3, 50, 260)
CASES = ("known answer 0", "known answer 1", "known answer 2", "counter layout", "words TransE", "words ComplEx",
         "words DistMult", "words 2^62 fit", "wrong n_slots code", "ConvE code", "neg_bound unread by ComplEx",
         "neg extremes", "hot extremes", "uniform below 1", "normal finite")
RULES = (("words ConvE", "keyed draws serve TransE, ComplEx and DistMult"), ("words decreasing row_off", "bad row_off"),
         ("words beyond int64", "word count beyond int64"), ("words negative epochs", "negative epochs"),
         ("words batch_size 0", "batch_size must be positive"), ("null request", "missing request"),
         ("wrong n_slots", "n_slots differs from the batch's"), ("null slot_key", "missing keys"),
         ("null init_key", "missing keys"), ("ConvE", "keyed draws serve TransE, ComplEx and DistMult"),
         ("neg_bound 0", "neg_bound must be in [1, 2^31]"), ("neg_bound 2^31 + 1", "neg_bound must be in [1, 2^31]"),
         ("int64", "word count beyond int64"))


@pytest.fixture(scope="module")
def restated():
    """The sweep by the restatement, computed once: (int32 words, [(kind, float32 row)])."""
    ints = []
    for R in RS:
        for E in ES:
            key = SLOT_KEY + 1000003 * R + E
            for n in NS:
                ints.append(kr.slot_rng("TransE", key, R, E, 64, n))
            ints.append(kr.slot_rng("ComplEx", key, R, E, 64))
    rows = []
    for d in DS:
        rows.append(("uniform", kr.x0_uniform(INIT_KEY + d, d, np.float32(1e-3))))
        rows.append(("normal", kr.x0_normal(INIT_KEY + d, d, np.float32(np.sqrt(2.0 / (d + 1))))))
    return np.concatenate(ints).astype(np.int32), rows


def test_known_answers_in_the_restatement():
    for ctr, key, out in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                          ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                          ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                           (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert tuple(int(v) for v in kr.philox(*ctr, *key)) == out


@pytest.mark.parametrize("target", ["keyed", "keyed_asan"])
def test_keyed_driver(target, restated, tmp_path):
    r = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    path = str(tmp_path / "sweep.bin")
    p = subprocess.run([os.path.join(ROOT, "build", "san", target), path], capture_output=True, text=True, env=env,
                       timeout=120)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-4000:]
    for marker in ("AddressSanitizer", "LeakSanitizer", "runtime error"):
        assert marker not in p.stderr, p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "0 failures" and "FAIL" not in p.stdout, p.stdout
    assert "good: ok" in lines, p.stdout
    for case in CASES:
        assert f"{case}: ok" in lines, (case, p.stdout)
    for case, msg in RULES:
        assert f"{case}: {msg}" in lines, (case, p.stdout)
    # the driver's sweep against the restatement
    ints, rows = restated
    got = np.fromfile(path, dtype=np.int32)
    n_float = sum(len(r) for _, r in rows)
    assert f"sweep: {len(ints) + n_float} values" in lines and len(got) == len(ints) + n_float
    assert np.array_equal(got[:len(ints)], ints)
    at = len(ints)
    for kind, want in rows:
        have = got[at:at + len(want)].view(np.float32)
        at += len(want)
        if kind == "uniform":
            assert np.array_equal(have.view(np.int32), want.view(np.int32))
        else:
            dist = kr.ulp_distance(have, want)
            print(f"normal d={len(want)}: {int((dist > 0).sum())} of {len(want)} elements differ, max {int(dist.max())} ulp")
            assert dist.max() <= 1
