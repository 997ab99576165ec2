"""CPU companion of test_topk_gpu.py's post-trained cases (topk_cases.py): the oracle alone,
through the list-serving stand-ins, meets every property the device is held to, and the
hard-coded picks do what they were picked for."""
import pytest

import topk_cases as tc
import width_cases as wc


@pytest.mark.parametrize("case", tc.CASES, ids=wc.ids(tc.CASES))
def test_oracle_meets_the_list_checks(case):
    slots, model = tc.run(case, tc.oracle_ctx)
    assert len(slots) == 6
    near, far = tc.check_lists(slots, model, model.ctx)
    # the guard against a vacuous rank invariant: both sides of K occur
    assert near >= 1 and far >= 1, (near, far, [s["rank"] for s in slots])


def test_near_objects_are_the_documented_picks():
    assert tc.pick_near_objects() == tc.NEAR_OBJECT
