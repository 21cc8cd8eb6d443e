#!/bin/bash
# One line per GPU kernel: a hash of its device assembly and its demangled name.  Two trees whose lines are equal
# compile to the same kernels, instruction for instruction and with the same kernel descriptors (registers, scratch,
# LDS, occupancy inputs) -- the check for a refactor that only moves code (no GPU needed):
#   scripts/kernel_isa_digest.sh > new.txt                      every shared-sweep object of this tree
#   scripts/kernel_isa_digest.sh -C ../old/syzgydb_amd/csrc kernels_mq.hip kernels_mq.hip:-DSZG_MQ_PART=1 > old.txt
#   scripts/kernel_isa_digest.sh kernels_scan.hip:-DSZG_QBITS=8,-DSZG_SCAN_METRIC=1      (a width and a metric: required)
#   scripts/kernel_isa_digest.sh kernels_scan.hip:-DSZG_QBITS=8,-DSZG_SCAN_METRIC=1,-DSZG_GROUP_FORM=3   (a G > 1 form)
#   scripts/kernel_isa_digest.sh kernels_scan_merge.hip                                  (the list-merge kernels)
#   scripts/kernel_isa_digest.sh kernels_scan_mx.hip:-DSZG_SCAN_METRIC=1,-fno-slp-vectorize,-DSZG_MX_NO_SLP   (MX_FLAGS)
# An argument is SOURCE[:FLAG[,FLAG...]], compiled with the build's flags (CXXFLAGS of syzgydb_amd/csrc/Makefile) plus
# --cuda-device-only -S.  The text of a kernel is its instructions (label to .Lfunc_end) and its .amdhsa_kernel block;
# the function index inside local labels (.LBB<n>_<m>, .Lfunc_end<n>, .LJTI<n>_<m>, and BB<n>_<m> in the loop comments), which
# depends on the order of the functions in the file, is taken out before hashing, and runs of blanks become one (the
# comment column moves with a label's length).  The lines are sorted by name.
set -euo pipefail
dir="$(dirname "$0")/../syzgydb_amd/csrc"
if [ "${1:-}" = -C ]; then dir=$2; shift 2; fi
cd "$dir"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
CXXFLAGS=${CXXFLAGS:--O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function}
if [ $# -eq 0 ]; then
    set -- kernels_mq.hip kernels_mq_bf16.hip:-DSZG_ROW_BITS=32 kernels_mq_bf16.hip:-DSZG_ROW_BITS=16 \
        kernels_mq_bf16.hip:-DSZG_ROW_BITS=64 kernels_mq_bf16d.hip \
        kernels_mq_i8.hip:-DSZG_ROW_BITS=8 kernels_mq_i8.hip:-DSZG_ROW_BITS=4
fi
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
i=0
for spec in "$@"; do
    src=${spec%%:*}
    flags=
    if [ "$spec" != "$src" ]; then flags=${spec#*:}; fi
    echo "$HIPCC $CXXFLAGS ${flags//,/ } ${VFLAGS:-} --cuda-device-only -S $src -o $tmp/$i.s"
    i=$((i + 1))
done | xargs -P "${JOBS:-8}" -I{} sh -c '{}'
cat "$tmp"/*.s | python3 -c '
import hashlib, re, subprocess, sys
lines = sys.stdin.read().split("\n")
kernels = [m.group(1) for ln in lines for m in [re.match(r"\s*\.amdhsa_kernel (\S+)", ln)] if m]
text = {k: [] for k in kernels}
cur = None
for ln in lines:
    m = re.match(r"(\S+):", ln)
    if cur is None and m and m.group(1) in text:
        cur = m.group(1)
    m = re.match(r"\s*\.amdhsa_kernel (\S+)", ln)
    if m:
        cur = m.group(1)
    if cur is not None:
        text[cur].append(re.sub(r"\s+", " ", re.sub(r"\b(LBB|BB|Lfunc_end|LJTI)\d+", r"\1", ln)))
        if re.match(r"\.Lfunc_end\d+:", ln) or ".end_amdhsa_kernel" in ln:
            cur = None
names = subprocess.run(["c++filt"], input="\n".join(kernels), capture_output=True, text=True).stdout.split("\n")
out = []
for k, name in zip(kernels, names):
    name = re.sub(r"^void |szg::\(anonymous namespace\)::", "", name).split("(")[0]
    out.append("%s  %s" % (hashlib.sha256("\n".join(text[k]).encode()).hexdigest()[:16], name))
print("\n".join(sorted(out, key=lambda s: s.split("  ", 1)[1])))
'
