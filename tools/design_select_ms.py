#!/usr/bin/env python3
"""Device time of the design selection next to the pick call, on one record.

The benchmark's workload (synthetic(length), MFE) is recorded for --steps steps
under an annealing cycle of --cycle steps; then Engine.picks and Engine.designs
run --repeat times each on that record and the HIP-event times
(adx_last_pick_ms, adx_last_design_ms) are printed as one JSON line per call,
then a summary line with the histogram's pair comparisons per second.

    python tools/design_select_ms.py [--walkers 4096] [--length 100] [--steps 300] [--cycle 50]
                                     [--window 25] [--radius 3] [--max-designs 100] [--repeat 3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--cycle", type=int, default=50)
    ap.add_argument("--window", type=int, default=25)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--max-designs", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--fold", choices=("mfe", "pf"), default="mfe")
    a = ap.parse_args()
    from addapt_amd import native, workloads

    tmpl, active = workloads.synthetic(a.length)
    apt = (workloads.THEO_SEQ, workloads.THEO_FOLD, native.theo_energy())
    th = native.make_thermostat("annealing", t_hi=5.0, t_lo=0.0, cycle_len=a.cycle)
    eng = native.Engine(tmpl, [active], workloads.config_objective(a.length, bppm=False), aptamer=apt, thermostat=th,
                        fold_mode=a.fold)
    eng.walkers_init(list(range(a.walkers)), workloads.walker_sequences(tmpl, [active], a.walkers, seed_base=1000))
    eng.record(a.steps)
    run_ms, left = 0.0, a.steps
    while left > 0:
        n = min(300, left)
        eng.run_steps(n)
        run_ms += eng.last_kernel_ms()
        left -= n
    rows = []
    for k in range(a.repeat):
        eng.picks(a.window)
        pick_ms, replay_ms = eng.last_pick_ms()
        designs, hist, n_picks = eng.designs(a.window, a.radius, a.max_designs)
        select_ms, hist_ms = eng.last_design_ms()
        rows.append((pick_ms, replay_ms, select_ms, hist_ms))
        print(json.dumps({"call": k, "pick_ms": pick_ms, "replay_ms": replay_ms, "design_select_ms": select_ms,
                          "design_hist_ms": hist_ms, "picks": n_picks, "designs": len(designs),
                          "covered": sum(d[4] for d in designs), "largest": max([d[4] for d in designs] or [0]),
                          "most_walkers": max([d[5] for d in designs] or [0])}))
    best = [min(r[i] for r in rows) for i in range(4)]
    pairs = int(hist.sum())
    print(json.dumps({"walkers": a.walkers, "length": a.length, "fold": a.fold, "steps": a.steps, "cycle": a.cycle,
                      "window": a.window, "radius": a.radius, "max_designs": a.max_designs, "run_kernel_ms": run_ms,
                      "min_pick_ms": best[0], "min_replay_ms": best[1], "min_design_select_ms": best[2],
                      "min_design_hist_ms": best[3], "pairs": pairs,
                      "pairs_per_second": pairs / (best[3] * 1e-3) if best[3] > 0 else None,
                      "pair_hist": {str(d): int(c) for d, c in enumerate(hist) if c}}))


if __name__ == "__main__":
    main()
