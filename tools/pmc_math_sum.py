"""Per-kernel sums of a rocprofv3 --pmc run's counter_collection csv (tools/pmc_math.sh):
usage: python3 tools/pmc_math_sum.py RUN_DIR OUT.json — {kernel: {counter: sum over its launches}}, the
kernel names cut at their template arguments' end, plus SQ_VALU_MFMA_BUSY_CYCLES per SQ_BUSY_CYCLES (the two
counters sum over different units, so the ratio compares kernels and maths, it is not a fraction) and
VALU instructions per MFMA."""
import csv
import glob
import json
import os
import re
import sys

rows = {}
for f in glob.glob(os.path.join(sys.argv[1], "**", "*counter_collection.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        k = re.sub(r"\(.*$", "", r["Kernel_Name"]).replace("void spw::", "")[:90]
        d = rows.setdefault(k, {"launches": set()})
        d["launches"].add(r.get("Dispatch_Id"))
        d[r["Counter_Name"]] = d.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
out = {}
for k, d in sorted(rows.items(), key=lambda kv: -kv[1].get("SQ_BUSY_CYCLES", 0)):
    d["launches"] = len(d["launches"])
    if d.get("SQ_BUSY_CYCLES"):
        d["mfma_busy_per_busy_cycle"] = round(d.get("SQ_VALU_MFMA_BUSY_CYCLES", 0) / d["SQ_BUSY_CYCLES"], 4)
    if d.get("SQ_INSTS_MFMA"):
        d["valu_per_mfma"] = round(d.get("SQ_INSTS_VALU", 0) / d["SQ_INSTS_MFMA"], 2)
    out[k] = d
json.dump(out, open(sys.argv[2], "w"), indent=1)
for k, d in list(out.items())[:14]:
    print(f"{k[:70]:70s} n={d['launches']:3d} busy={d.get('SQ_BUSY_CYCLES', 0):.3e} mfma_busy/busy={d.get('mfma_busy_per_busy_cycle')} "
          f"mfma={d.get('SQ_INSTS_MFMA', 0):.3e} valu={d.get('SQ_INSTS_VALU', 0):.3e} lds={d.get('SQ_INSTS_LDS', 0):.3e}")
