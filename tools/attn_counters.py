"""Counters of the attn_f16x3_kernel dispatches of a `rocprofv3 --pmc` pass, per wave and as shares of the kernel's time.

  rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_VALU_MFMA_BUSY_CYCLES SQ_WAVE_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_INST_LDS \
            SQ_LDS_BANK_CONFLICT SQ_BUSY_CYCLES --kernel-include-regex attn_f16x3 -d DIR --output-format csv -- \
            python3 bench.py --gpus 1 --config C3 --steps 1 --warmup 0          (a pass of its own: no trace domain beside it)
  python tools/attn_counters.py DIR/.../counter_collection.csv

GRBM_GUI_ACTIVE is summed over the 8 XCDs: / 8 = cycles of the dispatch, and with the dispatch's own timestamps the clock.
SQ_VALU_MFMA_BUSY_CYCLES counts cycles per SIMD (a wave's 192 MFMAs of 32 cycles are 6 144 of them); SQ_WAVE_CYCLES,
SQ_ACTIVE_INST_VALU and SQ_WAIT_INST_LDS count in units of four cycles per wave, and ACTIVE_INST_VALU comes out as one unit per
vector instruction issued, the 192 MFMAs included (parent 3 908 per wave against 3 872 + 192 in its assembly, part of them in
branches not taken).  Waves = Grid_Size / 64: the dispatch is taken as full, so a call whose last windows are shorter than 129
frames shows fewer matrix cycles per wave than 6 144."""
import csv
import sys
from collections import defaultdict

rows = defaultdict(dict)
for r in csv.DictReader(open(sys.argv[1], newline="")):
    if "attn_f16x3" not in r["Kernel_Name"]:
        continue
    d = rows[int(r["Dispatch_Id"])]
    d[r["Counter_Name"]] = float(r["Counter_Value"])
    d["grid"], d["ns"] = int(r["Grid_Size"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
    d["relpos"] = "<true>" in r["Kernel_Name"]
groups = defaultdict(list)
for d in rows.values():
    groups[(d["grid"], d["relpos"])].append(d)
for (grid, relpos), ds in sorted(groups.items()):
    n = len(ds)
    mean = lambda k: sum(d.get(k, 0.0) for d in ds) / n                                    # noqa: E731
    waves, cyc, ms = grid / 64, mean("GRBM_GUI_ACTIVE") / 8, mean("ns") * 1e-6
    simd_cycles = cyc * 1024                                                                # 256 CUs x 4 SIMDs
    print(f"grid {grid} ({grid // 256} workgroups{', bias instance' if relpos else ''}): {n} dispatches, {ms:.3f} ms under the counters, "
          f"{cyc / 1e6:.3f} M cycles, clock {cyc / (ms * 1e-3) / 1e9:.3f} GHz")
    print(f"  matrix pipe busy {100 * mean('SQ_VALU_MFMA_BUSY_CYCLES') / simd_cycles:.1f} % of the SIMD cycles "
          f"({mean('SQ_VALU_MFMA_BUSY_CYCLES') / waves:.0f} cycles per wave)")
    valu, life, lds = mean("SQ_ACTIVE_INST_VALU") / waves, mean("SQ_WAVE_CYCLES") / waves, mean("SQ_WAIT_INST_LDS") / waves
    print(f"  per wave: lifetime {4 * life:.0f} cycles, {valu:.0f} vector instructions issued ({valu - 192:.0f} outside the matrix pipe: "
          f"{4 * (valu - 192):.0f} cycles of issue, {100 * (valu - 192) / life:.1f} % of the lifetime), waiting on LDS {4 * lds:.0f} cycles ({100 * lds / life:.1f} %)")
    print(f"  vector issue of the two waves of a SIMD (4 cycles an instruction) {100 * 4 * mean('SQ_ACTIVE_INST_VALU') / simd_cycles:.1f} % of the SIMD cycles; "
          f"LDS bank conflict cycles {mean('SQ_LDS_BANK_CONFLICT'):.0f}; SQ busy cycles {mean('SQ_BUSY_CYCLES') / 1e6:.1f} M")
