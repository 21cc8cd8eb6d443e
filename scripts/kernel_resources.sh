#!/bin/bash
# Register / scratch / LDS use of every kernel of one object of the build:
#   scripts/kernel_resources.sh mq i8 4       -> kernels_mq_i8.hip -DSZG_ROW_BITS=4 (the 4-bit int8 sweeps)
#   scripts/kernel_resources.sh mq bf16 32    -> kernels_mq_bf16.hip -DSZG_ROW_BITS=32    (also: mq bf16d)
#   scripts/kernel_resources.sh mq select     -> kernels_mq.hip (the selection kernels)
#   scripts/kernel_resources.sh scan 32 [m]   -> kernels_scan.hip -DSZG_QBITS=32 -DSZG_SCAN_METRIC=m (the width is
#                                                required; m: 1 = cosine, the default, 0 = Euclidean): the G = 1 kernels
#   VFLAGS=-DSZG_GROUP_FORM=3 scripts/kernel_resources.sh scan 8
#                                             -> instead, the metric's G > 1 kernels of one form (bit 0: two planes, bit 1:
#                                                resident norms)
#   scripts/kernel_resources.sh merge         -> kernels_scan_merge.hip (the list-merge kernels)
#   scripts/kernel_resources.sh scan mx 1     -> kernels_scan_mx.hip -DSZG_SCAN_METRIC=1 (the matrix sweep, cosine)
#   VFLAGS=-DSZG_MX_COLLECT scripts/kernel_resources.sh scan mx 1
#                                             -> its collect form (radius searches through the sketch)
#   scripts/kernel_resources.sh sample        -> kernels_sample_mx.hip (the sample pass of top-k through the sketch)
#   scripts/kernel_resources.sh exact         -> kernels_exact.hip (re-rank, page-in, row gather, ...)
#   scripts/kernel_resources.sh prep          -> kernels_query_prep.hip (a sketch batch's queries prepared on the card)
#   scripts/kernel_resources.sh mask          -> kernels_mask.hip (device-resident filter masks)
#   scripts/kernel_resources.sh column        -> kernels_column.hip (resident metadata columns)
#   scripts/kernel_resources.sh column carry  -> kernels_column_carry.hip (columns carried across compaction / reorder)
# (hipcc -Rpass-analysis=kernel-resource-usage, device code only; no GPU needed)
set -euo pipefail
cd "$(dirname "$0")/../syzgydb_amd/csrc"
kind=${1:-mq}; part=${2:-i8}
if [ "$kind" = scan ] && [ "$part" = mx ]; then src=kernels_scan_mx.hip; def="-DSZG_SCAN_METRIC=${3:-1} -fno-slp-vectorize -DSZG_MX_NO_SLP"   # (the Makefile's MX_FLAGS)
elif [ "$kind" = scan ]; then src=kernels_scan.hip; def="-DSZG_QBITS=${2:?row width (4, 8, 16, 32, 64) or mx} -DSZG_SCAN_METRIC=${3:-1}"
elif [ "$kind" = sample ]; then src=kernels_sample_mx.hip; def=
elif [ "$kind" = merge ]; then src=kernels_scan_merge.hip; def=
elif [ "$kind" = exact ]; then src=kernels_exact.hip; def=-ffp-contract=off
elif [ "$kind" = prep ]; then src=kernels_query_prep.hip; def=-ffp-contract=off
elif [ "$kind" = mask ]; then src=kernels_mask.hip; def=
elif [ "$kind" = column ] && [ "$part" = carry ]; then src=kernels_column_carry.hip; def=
elif [ "$kind" = column ]; then src=kernels_column.hip; def=
elif [ "$part" = select ]; then src=kernels_mq.hip; def=
elif [ "$part" = bf16d ]; then src=kernels_mq_bf16d.hip; def=
else src=kernels_mq_$part.hip; def=-DSZG_ROW_BITS=${3:?row width}; fi
/opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 $def ${VFLAGS:-} --cuda-device-only -c $src -o /dev/null \
    -Rpass-analysis=kernel-resource-usage 2>&1 | python3 -c '
import re, sys
name = None; row = {}
for ln in sys.stdin:
    m = re.search(r"Function Name: (\S+)", ln)
    if m:
        name = m.group(1); row = {}
    for key in ("VGPRs:", "AGPRs", "ScratchSize", "VGPRs Spill", "SGPRs Spill", "Occupancy", "LDS Size"):
        m = re.search(re.escape(key) + r".*?(\d+)", ln)
        if m and name: row[key] = int(m.group(1))
    if "LDS Size" in ln and name:
        import subprocess
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        dem = re.sub(r"szg::\(anonymous namespace\)::", "", dem).split("(")[0]
        print("%-64s vgpr %3d agpr %3d scratch %4d B  vgpr-spill %3d  lds %5d B  occupancy %d" % (
            dem[:64], row.get("VGPRs:", -1), row.get("AGPRs", 0), row.get("ScratchSize", 0), row.get("VGPRs Spill", 0), row.get("LDS Size", 0),
            row.get("Occupancy", 0)))
        name = None
'
