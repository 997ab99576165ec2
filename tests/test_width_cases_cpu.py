"""CPU companion of test_gpu_widths.py: the case table is complete and its checks decide.

* Completeness: every width the kernels are compiled for (the ``dbs[]`` list of cx_pick_db in
  kp_complex.hip, the ``case`` labels of KP_DB_DISPATCH in kp_attn3.hpp from the narrowest width
  kp_conve.hip dispatches with, the (VPL, NT) launches of kp_transe.hip) has a case in
  width_cases.py or a named test elsewhere in the GPU suite.
* The rank rule is not vacuous: on the oracle side of every case, every slot's bounds are at
  most one apart, three quarters of a case's slots admit one rank only, and the oracle's own
  rank lies inside (a condition on the inputs: seeds and scales are chosen for it).
* The host protocol accepts the direct-call batches and the tiny graphs without a device.
"""
import os
import re

import numpy as np
import pytest

import width_cases as wc

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "kelpie_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _compiled_dbs():
    m = re.search(r"int cx_pick_db\(int dim\) \{\s*static const int dbs\[\] = \{([^}]*)\};", _source("kp_complex.hip"))
    assert m, "cx_pick_db's dbs[] initialiser not found"
    return tuple(int(v) for v in m.group(1).split(","))


def _dispatch_dbs():
    """The case labels of KP_DB_DISPATCH, the one switch over the compiled widths."""
    m = re.search(r"#define KP_DB_DISPATCH\(DBV, DB_MIN, MSG, \.\.\.\)(.*?)default:", _source("kp_attn3.hpp"), re.S)
    assert m, "KP_DB_DISPATCH not found"
    return tuple(int(v) for v in re.findall(r"KP_DB_CASE\((\d+), DB_MIN, __VA_ARGS__\)", m.group(1)))


def _dispatch_min(name, message):
    """The narrowest width `name` dispatches with: one value in all of its KP_DB_DISPATCH uses."""
    src = _source(name)
    mins = re.findall(r'KP_DB_DISPATCH\([^,;]+, (\d+),\s*"' + re.escape(message) + '"', src)
    assert mins and len(mins) == src.count("KP_DB_DISPATCH(") and len(set(mins)) == 1, (name, mins)
    return int(mins[0])


def _conve_dbs():
    lo = _dispatch_min("kp_conve.hip", "ConvE: unsupported padded dimension")
    return sorted(db for db in _dispatch_dbs() if db >= lo)


# --------------------------------------------------------------------------- completeness
def test_pick_db_restates_the_library():
    assert _compiled_dbs() == wc.DBS
    assert _dispatch_dbs() == wc.DBS, "KP_DB_DISPATCH's cases differ from cx_pick_db's list"
    assert _dispatch_min("kp_complex.hip", "ComplEx / DistMult: unsupported padded dimension") == 1
    assert [wc.pick_db(w) for w in (1, 16, 17, 32, 33, 64, 65, 128, 129, 208, 209, 256, 257, 400, 401)] == \
        [1, 1, 2, 2, 4, 4, 8, 8, 13, 13, 16, 16, 25, 25, -1]


def test_every_compiled_attention_width_has_a_gpu_case():
    dbs = _compiled_dbs()
    conve = _conve_dbs()
    assert conve and set(conve) <= set(dbs)
    smallest = wc.pick_db(60)  # ConvE's smallest image, 20 x 3
    assert conve == [db for db in dbs if db >= smallest], "a ConvE width that is not dispatched (or the reverse)"
    wanted = [(m, db) for m in ("ComplEx", "DistMult") for db in dbs] + [("ConvE", db) for db in conve]
    have = {(c["model"], c["db"]) for c in wc.SWEEP if "db" in c}
    for model, db in wanted:
        mode = wc.ATTN_MODE[model]
        assert (model, db) in have or (model, mode, db) in wc.COVERED_BY, \
            f"kp_attn3<{db}, {mode}> ({model}) has no GPU case: add one to width_cases.SWEEP"
    # an entry of COVERED_BY names a test that exists
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    for where in wc.COVERED_BY.values():
        fname, test = where.split("::")
        with open(os.path.join(tests_dir, fname)) as f:
            assert f"def {test.split('[')[0]}(" in f.read(), where
    # the fp32 contraction (KP_ATTN=f32) has its own per-DB dispatch: ComplEx and ConvE cases
    # are run through it too, and ComplEx alone reaches every DB
    assert {c["db"] for c in wc.SWEEP if c["model"] == "ComplEx"} | {1, 25} >= set(dbs)


def test_every_transe_launch_has_a_gpu_case():
    src = _source("kp_transe.hip")
    launches = sorted({(int(v), int(t)) for v, t in re.findall(r"TE_STAGE\((\d+), (\d+)\);", src)})
    assert launches == [(1, 512), (1, 1024), (2, 512)], launches
    have = {c["inst"] for c in wc.SWEEP if c["model"] == "TransE"}
    # (1, 512) is reached only through the KELPIE_TE_NT diagnostic, never by a dimension
    assert have == {(1, 1024), (2, 512)}
    assert wc.te_inst(256) == (1, 1024) and wc.te_inst(257) == (2, 512) and wc.te_inst(512) == (2, 512)
    assert any(c["hub"] and c["inst"] == (2, 512) for c in wc.SWEEP), "the unstaged VPL = 2 kernel has no case"
    assert any(c["norm"] == 1 and c["inst"] == (2, 512) for c in wc.SWEEP)
    # widths that are no multiple of 16 (dp > d) on both instantiations
    assert any(c["dim"] % 16 and c["inst"] == inst for inst in have for c in wc.SWEEP if c["model"] == "TransE")


def test_case_ids_are_unique_and_edges_are_complete():
    all_cases = wc.SWEEP + wc.EDGES + wc.QUERIES
    assert len(set(wc.ids(all_cases))) == len(all_cases)
    assert sorted({c["n_ent"] for c in wc.EDGES if c["model"] == "ComplEx"}) == [31, 32, 33, 512, 513]
    assert sorted({c["nq"] for c in wc.QUERIES}) == [1, 16, 17, 64, 65]
    for nq, (slots, k) in wc.NQ_SPLIT.items():
        assert slots * k == nq
    for n in (517, 31, 32, 33, 512, 513):
        assert wc.graph(n)[1].num_entities == n


# --------------------------------------------------------------------------- the rank rule decides
def test_rank_bounds_rule():
    s = np.array([0.5, 0.50004, 0.3, 0.7, 0.49996, 0.9], np.float32)
    # maximizer, target entity 0 (counted: not filtered): 0.7 and 0.9 above, two within delta
    assert wc.rank_bounds(s, s[0], [], 0) == (3, 5)
    assert wc.rank_bounds(s, s[0], [0, 5], 0) == (1, 3)  # a filtered object is left out
    assert wc.rank_bounds(s, s[0], [1, 4], 0) == (3, 3)
    # minimizer: the object is restored even when filtered
    assert wc.rank_bounds(s, s[0], [0, 5], 0, minimizer=True) == (2, 4)
    assert wc.rank_bounds(s, s[0], [1, 4], 0, minimizer=True) == (2, 2)


@pytest.mark.parametrize("case", wc.SWEEP + wc.EDGES + wc.QUERIES, ids=wc.ids(wc.SWEEP + wc.EDGES + wc.QUERIES))
def test_rank_rule_is_not_vacuous(case):
    """Also the host protocol: the tiny graphs and the direct-call batches go through the
    engine's packing, the batch layout and the oracle-backed context with no device."""
    ref = wc.reference(case)
    wc.check_vacuity(ref)
    if "nq" in case:
        assert len(ref) == wc.NQ_SPLIT[case["nq"]][0]
    elif case["hub"]:
        assert len(ref) == 2 and min(b["n_rows"] for b in ref) == wc.hub_rows(case) > 682
    else:
        assert len(ref) == 6  # two subjects: a base slot and two candidates each
    if case["model"] == "ConvE":
        # no target in the saturated sigmoid (test_conve_saturated_sigmoid_ties owns that regime)
        assert all(0.01 < b["score"] < 0.99 for b in ref), [b["score"] for b in ref]
    for b in ref:
        assert np.isfinite(b["x"]).all() and np.isfinite(b["score"])


def test_direct_call_batch_layout():
    """query_batch: every row involves the kelpie entity, a slot has exactly k distinct
    relations with the kelpie entity as head, and its inverses' heads are frozen."""
    for case in wc.QUERIES:
        model = wc.make_model(case)
        hp, x0, row_off, rows, rng_off, rng, pred, filt_off, filt = wc.query_batch(case, model)
        K = model.dataset.num_entities
        n_slots, k = wc.NQ_SPLIT[case["nq"]]
        assert len(row_off) == n_slots + 1 and x0.shape == (n_slots, model.dimension)
        nq = 0
        for s in range(n_slots):
            r = rows[row_off[s]:row_off[s + 1]]
            assert ((r[:, 0] == K) ^ (r[:, 2] == K)).all()
            nq += len({int(v) for v in r[r[:, 0] == K][:, 1]})
            assert int(pred[s][0]) == K and len(r) <= hp.batch_size
        assert nq == case["nq"]
        assert rng_off[-1] == len(rng) and (len(rng) > 0) == (model.name == "ConvE")
