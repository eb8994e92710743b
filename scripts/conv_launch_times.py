"""per-launch mean duration of the fused tokenizer convolutions (24 per encoder pass, in launch order) from a rocprofv3 kernel trace"""
import csv, sys
rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        n = r.get("Kernel_Name") or r.get("Name") or ""
        if "conv_slab" in n:
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), "pool" if "ELb1ELb1" in n or "true, true" in n else "full"))
rows.sort()
npass = len(rows) // 24
print(f"# {len(rows)} conv_slab launches = {npass} encoder passes of 24; mean / min us per launch index")
for i in range(24):
    d = [rows[p * 24 + i][1] / 1e3 for p in range(1, npass)] or [0.0]   # (first pass = warm-up)
    print(f"{i:2d} {rows[i][2]:4s} mean {sum(d) / len(d):8.1f} min {min(d):8.1f}")
others = {}
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        n = r.get("Kernel_Name") or ""
        for k in ("avgpool_stats_kernel", "nchw_to_nhwc_kernel", "conv_in_direct_kernel"):
            if k in n:
                others.setdefault(k, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for k, d in others.items():
    print(f"{k}: {len(d)} launches, mean {sum(d) / len(d):.1f} us, total {sum(d) / 1e3:.2f} ms")
