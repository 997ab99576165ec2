"""What ``attributions`` cost (ANALYSIS TOOL; runs on the GPU, reads the
committed fixtures only).

    python tools/attrib_cost.py [--workload complex-fb15k237-sufficient] [--pairs 4]

One singleton batch of the workload (bench.py's first prediction, its candidates and conversion
entities) on one context, without and with attributions alternating on the same box, ``pairs``
counted pairs after one pair that warms the context: device ms per batch and per optimizer step
(kp_last_timing), the medians, their difference, and the launches a call with attributions adds.
The relevances of the two are compared bit for bit.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# what a call with attributions launches beyond the call without (kp_complex.hip): per step
# kp_cx_attrib (kp_cx_update runs in its ATTRIB form, not a further launch); per batch
# kp_cx_attrib_c, kp_cx_attrib_delta, one memset of the results and one copy of the initial rows
ADDED = {"launches_per_step": 1, "launches_per_batch": 2, "memsets_per_batch": 1, "device_copies_per_batch": 1,
         "downloads_per_batch": 3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="complex-fb15k237-sufficient")
    ap.add_argument("--pairs", type=int, default=4)
    a = ap.parse_args()
    import bench
    from kelpie_amd import NecessaryPostTrainingEngine, SufficientPostTrainingEngine
    wl = bench.WORKLOADS[a.workload]
    ds, model, _ = bench.build(wl, 0, 0)
    cls = SufficientPostTrainingEngine if wl["mode"] == "sufficient" else NecessaryPostTrainingEngine
    eng = cls(model, ds, wl["hp"])
    pred = bench.pick_preds(ds, 1, seed=1234)[0]
    cands = [[c] for c in bench.candidates_of(ds, pred, wl["candidates"])]
    if wl["mode"] == "sufficient":
        bench.seed_all(42)
        eng.entities_to_convert = eng.select_entities_to_convert(pred, wl["convert"], 200)
    runs = {False: [], True: []}
    rels = {}
    for i in range(a.pairs + 1):
        for on in (False, True):
            eng.attributions = on
            eng.set_cache()
            bench.seed_all(42)
            rels[on] = eng.compute_relevance_batch(pred, cands)
            st = eng.last_batch_stats
            if i:  # the first pair warms both paths
                runs[on].append((st["device_s"], st["hot_launches"], st["slots"], st["rows"]))
    out = {"workload": a.workload, "pairs": a.pairs, "relevances_equal": rels[False] == rels[True], "added": ADDED}
    for on, rs in runs.items():
        dev = sorted(r[0] for r in rs)[len(rs) // 2]
        out["with" if on else "without"] = {
            "slots": rs[0][2], "rows": rs[0][3], "steps": rs[0][1], "device_ms": round(dev * 1e3, 3),
            "ms_per_step": round(dev * 1e3 / max(1, rs[0][1]), 4), "device_ms_all": [round(r[0] * 1e3, 3) for r in rs]}
    out["added_ms_per_batch"] = round(out["with"]["device_ms"] - out["without"]["device_ms"], 3)
    out["with_over_without"] = round(out["with"]["device_ms"] / out["without"]["device_ms"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
