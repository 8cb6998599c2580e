#!/bin/bash
# Cumulative kernel time of k_bgzf_deflate's phases: the library is built with -DVMX_BGZF_STOP=k (the kernel ends after phase k: 1 load +
# byte histogram + CRC, 2 matching, 3 parse, 4 histograms + Huffman tables + block header; csrc/k_bam.hip), and tools/bam_bench.py kernels
# runs on each build under rocprofv3 kernel tracing. Phase k costs time(k) - time(k-1); the full kernel is the in-tree build.
#     bash tools/bam_deflate_phases.sh OUT_DIR [GB]
set -e -o pipefail
OUT=${1:?output directory}; GB=${2:-0.5}
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
mkdir -p "$OUT"; LIBS=$(mktemp -d)
for k in 1 2 3 4; do
    (cd "$ROOT" && VMX_EXTRA_FLAGS="-DVMX_BGZF_STOP=$k" timeout -k 10 600 python3 -m vacmap_amd.build --force > "$OUT/build_stop$k.log" 2>&1)
    cp "$ROOT/vacmap_amd/libvacmapx.so" "$LIBS/libvacmapx_stop$k.so"
done
(cd "$ROOT" && timeout -k 10 600 python3 -m vacmap_amd.build --force > "$OUT/build_full.log" 2>&1)
for k in 1 2 3 4 full; do
    lib="$LIBS/libvacmapx_stop$k.so"; [ "$k" = full ] && lib="$ROOT/vacmap_amd/libvacmapx.so"
    VACMAPX_LIB="$lib" timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/stop$k" -o bam -- \
        python3 "$ROOT/tools/bam_bench.py" kernels --gb "$GB" > "$OUT/stop$k.log" 2>&1
    printf 'stop %s: ' "$k"; grep -h 'k_bgzf_deflate' "$OUT"/stop$k/*kernel_stats.csv | cut -d, -f1-4 | sed 's/(.*)"/"/'
done
rm -rf "$LIBS"
