#!/bin/bash
# First measurements of the frame check / decode path (recorded, not gated): decode frames/s beside the encode rate of one process
# (tools/decode_measure.py), per-kernel time from a kernel trace in a run of its own, and the kernels' registers / LDS from the ISA
# guard's summary of the linked library.   usage: tools/decode_first.sh [output file, default profiles/decode_first.txt]
set -e -o pipefail
cd "$(dirname "$0")/.."
out=${1:-profiles/decode_first.txt}
work=$(mktemp -d)
{
    echo "# tools/decode_first.sh: BASELINE configs[1] shape, buffers resident on the device"
    echo "## rates (one process)"
    timeout -k 10 300 python tools/decode_measure.py
    echo
    echo "## per-kernel time (rocprofv3 --kernel-trace --stats of the same script, a run of its own)"
    timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$work" -o dec -- python tools/decode_measure.py > "$work/run.log" 2>&1
    f=$(find "$work" -name "*kernel_stats.csv" | head -1)
    python - "$f" <<'PY'
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
print(f"{'kernel':60s} {'calls':>6s} {'total ms':>10s} {'mean ms':>9s} {'share %':>8s}")
for r in rows:
    print(f"{r['Name'][:60]:60s} {int(r['Calls']):6d} {float(r['TotalDurationNs']) / 1e6:10.3f} {float(r['AverageNs']) / 1e6:9.3f} {float(r['Percentage']):8.2f}")
PY
    echo
    echo "## registers / LDS of the linked library's kernels (tools/check_isa.py)"
    python tools/check_isa.py odr-audioenc_amd/libtoolame_dab_hip.so --no-fail | grep -E "kernel +vgpr|tl_unpack|tl_synth|tl_dec_carry|tl_frame_kernelILi1ELb0ELi2"
} > "$out.tmp"
mv "$out.tmp" "$out"
rm -rf "$work"
cat "$out"
