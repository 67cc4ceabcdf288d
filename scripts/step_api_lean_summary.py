#!/usr/bin/env python3
"""Condense a default-vs-lean session of scripts/step_api_bench.py (one JSON
line per run, with and without --lean) and the lean loop's FETCH_SIZE /
WRITE_SIZE summaries (scripts/pmc_summary.py) into the figures DESIGN §3
"Lean frames" quotes: median and spread (max - min) of the time per step,
the lean / default ratio, HBM fractions by contract bytes and by SURVEY
§8(d)'s nominal 200 B per env-step, and counter bytes against the contract.

  python scripts/step_api_lean_summary.py profiles/r07 > profiles/r07/summary.json
"""

import csv
import json
import os
import statistics
import sys

HBM_PEAK = 8e12  # B/s (MI355X)
SURVEY_BYTES = 200


def counter_kib(path, kernel):
    for r in csv.DictReader(open(path)):
        if kernel in r["Kernel_Name"]:
            return float(r["Average_Per_Dispatch"]), int(r["Dispatches"])
    raise SystemExit(f"{kernel} not in {path}")


def main():
    d = sys.argv[1]
    rows = [json.loads(line) for line in open(os.path.join(d, "step_api_lean.jsonl")) if line.strip()]
    out = {"timing": []}
    for n in sorted({r["n"] for r in rows}, reverse=True):
        e = {"n": n}
        for lean in (False, True):
            rs = [r for r in rows if r["n"] == n and bool(r.get("lean")) == lean]
            us = [r["ms_per_step"] * 1e3 for r in rs]
            med = statistics.median(us)
            by = sum(rs[0]["contract_bytes_per_env_step"].values())
            e["lean" if lean else "default"] = {
                "runs_us_per_step": [round(x, 3) for x in us], "median_us_per_step": round(med, 3),
                "spread_us": round(max(us) - min(us), 3),
                "host_us_per_step_median": round(statistics.median(r["host_us_per_step"] for r in rs), 2),
                "contract_bytes_per_env_step": by, "env_steps_per_s": n / (med * 1e-6),
                "contract_hbm_frac": round(n * by / (med * 1e-6) / HBM_PEAK, 4),
                "survey_200B_hbm_frac": round(n * SURVEY_BYTES / (med * 1e-6) / HBM_PEAK, 4)}
        e["lean_over_default"] = round(e["lean"]["median_us_per_step"] / e["default"]["median_us_per_step"], 4)
        e["byte_ratio"] = round(e["lean"]["contract_bytes_per_env_step"] / e["default"]["contract_bytes_per_env_step"], 4)
        e["gain_over_default_spread"] = round(
            (e["default"]["median_us_per_step"] - e["lean"]["median_us_per_step"]) / e["default"]["spread_us"], 1)
        out["timing"].append(e)
    fetch = os.path.join(d, "pmc_FETCH_SIZE.csv")
    if os.path.exists(fetch):
        n = max(r["n"] for r in rows)
        f, nd = counter_kib(fetch, "lean_closed_step_kernel")
        w, _ = counter_kib(os.path.join(d, "pmc_WRITE_SIZE.csv"), "lean_closed_step_kernel")
        b = (2 * f + w) * 1024 / n  # 2 x FETCH_SIZE: gfx950's half-count
        contract = next(sum(r["contract_bytes_per_env_step"].values()) for r in rows if r.get("lean"))
        out["counters"] = {"n": n, "dispatches": nd, "FETCH_SIZE_KiB": f, "WRITE_SIZE_KiB": w,
                           "bytes_per_env_step": round(b, 2), "contract_bytes_per_env_step": contract,
                           "ratio": round(b / contract, 4)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
