"""The launches of ONE set_data out of a rocprofv3 --kernel-trace CSV of `tools/resolve_ab.py once`: every dispatch from the
first k_data_in on, in start order, with its duration (profiles/resolve_set_data_kernels.txt)."""
import csv
import sys

rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
first = next(i for i, r in enumerate(rows) if "k_data_in" in r["Kernel_Name"])
tail = rows[first:]
t0 = int(tail[0]["Start_Timestamp"])
print(f"dispatches before set_data (create, prepare): {first}; dispatches of set_data: {len(tail)}")
for r in tail:
    s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
    name = r["Kernel_Name"].replace("void hprlp::", "").replace("hprlp::", "")[:60]
    print(f"  {name:<60s} grid {r.get('Grid_Size', '?'):>8s}  start +{(s - t0) / 1e3:8.1f} us  duration {(e - s) / 1e3:6.1f} us")
print(f"first start to last end: {(int(tail[-1]['End_Timestamp']) - t0) / 1e3:.1f} us")
