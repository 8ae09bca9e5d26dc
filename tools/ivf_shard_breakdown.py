"""Compaction / scan / merge microseconds per call of the sharded-IVF list scan, split by form, from the kernel trace of
`rocprofv3 --kernel-trace --output-format csv -- python tools/ivf_shard_bench.py ...` (profiles/ivf_shard_breakdown.txt).
A segmented scan right after compact_probes_kernel is the local form (wise_ivf_scan_local_f32), otherwise the plain one.

    python tools/ivf_shard_breakdown.py <dir>/<name>_kernel_trace.csv
"""
import csv, sys, collections, json
rows = list(csv.DictReader(open(sys.argv[1])))
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
# walk the dispatches: a seg scan right after compact_probes_kernel is the local form, otherwise the plain form; the
# merge_keys_kernel after a seg scan belongs to the same call
acc = collections.defaultdict(lambda: collections.defaultdict(list))
mode = None; key = None
for r in rows:
    n = r["Kernel_Name"]; t = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    blocks = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
    if "compact_probes_kernel" in n:
        mode = "local"; nq = blocks; acc_key = None
        pend = ("compact", t, nq); continue
    if "ip_scan_kernel" in n and "true>" in n:
        if mode != "local":
            mode = "plain"
        key = (blocks, int(r["LDS_Block_Size"]))
        if mode == "local":
            acc[(key, "local")]["compact_us"].append(pend[1])
        acc[(key, mode)]["scan_us"].append(t); continue
    if "merge_keys_kernel" in n and key is not None and mode is not None:
        acc[(key, mode)]["merge_us"].append(t)
        mode = None; continue
print("grid_blocks lds_bytes form: median us per call (calls)")
for (key, m), d in sorted(acc.items()):
    med = {k: sorted(v)[len(v) // 2] for k, v in d.items()}
    print(key[0], key[1], m, " ".join(f"{k}={med[k]:.1f}" for k in ("compact_us", "scan_us", "merge_us") if k in med), f"({len(d['scan_us'])})")
