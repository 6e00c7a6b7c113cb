"""Joint fits against several observations WITH priors: ms per iteration of tools/bench_observations.py's workloads
(O1, O2, O3) in three legs

  a  without a prior                   (scarlet_fit_observations_constrained, the existing entry point)
  b  with weights only                 (scarlet_fit_observations_prior: QuadraticPrior(sed_weight, morph_weight))
  c  with a full-plane morphology target on every component as well (the stream the contraction then reads:
     K H W 4 bytes per scene and iteration)

Each leg is timed `--repeats` times over `--iters` iterations.  Reported per config: the three lists, c - a of the
medians beside the bytes c adds, and the rate that implies against what profiles/prior_bench.json records for
k_prior_step, the separate pass a folded prior saves.  `--legs a` runs on a tree without the feature too (SCARLET_TREE
points at it); `--parent FILE` (repeatable) merges such a run's document: the branch's median of leg a must lie
within the spread of the parent's own runs; `--pool FILE` adds further leg-a runs of this tree, so that both sets span
several processes.  Writes one JSON document to --out."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.environ.get("SCARLET_TREE") or os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from bench_observations import CONFIGS, data          # noqa: E402  (the workloads, unchanged)

# weak against the scenes' constants (L_morph = 2 K C = 40 to 480, L_sed some tens): the fit stays the fit of leg a, every
# scene keeps iterating (raise_on_status), and the cost of a prior does not depend on the value of its weight
WEIGHTS = dict(sed=0.1, morph=1.0)


def run(name, cfg, leg, iters, warmup, repeats):
    import torch
    from scarlet_amd import _lib
    from scarlet_amd.batch import BlendBatch, ObservationBatch
    obs, w, diff, cen, sed0, morph = data(cfg)
    ol = []
    for (im, b0), ww in zip(obs, w):
        o = ObservationBatch(im, band0=b0, weights=ww)
        if diff is not None:
            o.set_diff_kernel(diff)
        ol.append(o)
    b = BlendBatch.from_observations(ol, cen, l0_thresh=cfg["l0"], mse_capacity=warmup + (repeats + 1) * iters + 2)
    b.set_state(sed0, morph)
    prior = None
    if leg != "a":
        import scarlet_amd as scarlet
        target = None
        if leg == "c":
            target = torch.as_tensor(morph).to(b.device)
        prior = scarlet.QuadraticPrior(sed_weight=WEIGHTS["sed"], morph_weight=WEIGHTS["morph"], morph_target=target)
    fit = (lambda n: b.fit(n, e_rel=0, check_every=0)) if prior is None else \
          (lambda n: b.fit(n, e_rel=0, check_every=0, prior=prior))
    fit(warmup)
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fit(iters)
        torch.cuda.synchronize()
        ms.append(round((time.perf_counter() - t0) * 1e3 / iters, 4))
    b.raise_on_status()
    # the library's own event recorder around the classes of the observation step (scarlet_profile_begin / _end_ex):
    # [0] the observations' gradient planes, [1] the contraction(s), the constants and the head, [2] the constraint
    # pipeline, [3] the convergence test
    names = ["planes", "contract_and_head", "source_update", "converge"]
    _lib.check(_lib.lib.scarlet_profile_begin(iters + 1))
    fit(iters)
    tot, its = (ctypes.c_double * 8)(), (ctypes.c_int64 * 8)()
    _lib.check(_lib.lib.scarlet_profile_end_ex(tot, its, None))
    return ms, {names[i]: round(tot[i] / iters, 4) for i in range(len(names)) if its[i]}


def prior_step_rate():
    """GB/s of k_prior_step as profiles/prior_bench.json records it (kernel trace, per config)"""
    path = os.path.join(os.path.dirname(HERE), "profiles", "prior_bench.json")
    try:
        k = json.load(open(path))["k_prior_step_from_kernel_trace"]
        return {name: v["GBps"] for name, v in k.items()}
    except (OSError, KeyError, ValueError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="O1,O2,O3")
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", action="append", default=[], help="JSON written by a --legs a run on the parent commit")
    ap.add_argument("--pool", action="append", default=[], help="JSON written by a further --legs a run on THIS tree: its "
                    "timings join leg a's (process-to-process variation is larger than the spread within a process)")
    ap.add_argument("--reuse", help="take the legs' timings from this earlier --out file instead of measuring (to merge "
                                    "parent runs made after it)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "observations_prior_bench.json"))
    a = ap.parse_args()
    legs = a.legs.split(",")
    doc = dict(tool="tools/bench_observations_prior.py", device="MI355X (gfx950)",
               legs="a scarlet_fit_observations_constrained (no prior); b scarlet_fit_observations_prior, weights only; "
                    "c the same with a full-plane morphology target on every component",
               iters=a.iters, warmup=a.warmup, weights=WEIGHTS, k_prior_step_GBps_recorded=prior_step_rate(), configs=[])
    parents = [json.load(open(p)) for p in a.parent]
    pooled = [json.load(open(p)) for p in a.pool]
    earlier = {c["config"]: c for c in json.load(open(a.reuse))["configs"]} if a.reuse else {}
    for name in a.configs.split(","):
        cfg = CONFIGS[name]
        r = dict(config=name, scenes=cfg["S"], K=cfg["K"], side=cfg["side"])
        for leg in legs:
            r["ms_per_iter_" + leg], r["class_ms_per_iter_" + leg] = \
                (earlier[name]["ms_per_iter_" + leg], earlier[name]["class_ms_per_iter_" + leg]) if a.reuse else \
                run(name, cfg, leg, a.iters, a.warmup, a.repeats)
        if "a" in legs:
            r["ms_per_iter_a"] = r["ms_per_iter_a"] + [ms for p in pooled for c in p["configs"] if c["config"] == name
                                                       for ms in c["ms_per_iter_a"]]
        if "a" in legs and "c" in legs:
            d = float(np.median(r["ms_per_iter_c"]) - np.median(r["ms_per_iter_a"]))
            r["c_minus_a_ms"] = round(d, 4)
            r["bytes_c_adds_per_iter"] = cfg["S"] * cfg["K"] * cfg["side"] ** 2 * 4
            r["implied_GBps"] = round(r["bytes_c_adds_per_iter"] / (d * 1e-3) / 1e9, 1) if d > 0 else None
            r["b_minus_a_ms"] = round(float(np.median(r["ms_per_iter_b"]) - np.median(r["ms_per_iter_a"])), 4) if "b" in legs else None
        pa = [ms for p in parents for c in p["configs"] if c["config"] == name for ms in c["ms_per_iter_a"]]
        if pa and "a" in legs:
            med = float(np.median(r["ms_per_iter_a"]))
            r["parent_ms_per_iter_a"] = pa
            r["a_median"] = round(med, 4)
            r["a_median_within_parent_spread"] = bool(min(pa) <= med <= max(pa))
        doc["configs"].append(r)
        print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
