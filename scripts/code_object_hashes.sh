#!/bin/bash
# Are the gfx950 code objects of the one-sweep scan's kernels the same bytes in two trees?  For a change that is meant to
# touch host code only (launchers, guards, routing, the build file): every kernel object is compiled in both trees with
# the command its own Makefile gives for it, plus --cuda-device-only, and the sha256 of the two code objects are compared.
#   scripts/code_object_hashes.sh /path/to/parent/tree [jobs] ["object.o ..."]  > table
# The objects: kernels_scan_merge, the ten by-width scan objects, the eight G > 1 objects, the twenty matrix-sweep
# objects and kernels_sample_mx.  It hashes bytes and nothing else; exit status 1 if any pair differs.  (No GPU needed.)
# Both sides compile from their own csrc/ with the same relative paths, into build_hashes/ there: the names the compiler
# gives kernels of internal linkage carry a hash of the command line, input and output paths included.
set -euo pipefail
here=$(cd "$(dirname "$0")/.." && pwd)
parent=$(cd "${1:?the parent tree}" && pwd)
jobs=${2:-8}
tmp=$(mktemp -d)
out=build_hashes
trap 'rm -rf "$tmp" "$parent/syzgydb_amd/csrc/$out" "$here/syzgydb_amd/csrc/$out"' EXIT
objs="kernels_scan_merge.o kernels_sample_mx.o"
for q in 4 8 16 32 64; do objs="$objs kernels_scan_q${q}c.o kernels_scan_q${q}e.o"; done
for f in 0 1 2 3; do objs="$objs kernels_scan_g8c$f.o kernels_scan_g8e$f.o"; done
for f in mx mxc mxs mxm mxms mxl mxls mxlm mxlms mxlc; do objs="$objs kernels_scan_${f}_c.o kernels_scan_${f}_e.o"; done
objs=${3:-$objs}
# one line per (tree, object): the Makefile's own command for ./object, its output renamed, device code only
for side in parent new; do
    tree=$parent; [ $side = new ] && tree=$here
    mkdir -p "$tree/syzgydb_amd/csrc/$out"
    for o in $objs; do
        cmd=$(make -s -n -B -C "$tree/syzgydb_amd/csrc" "./$o" | grep -- "-o $o\$\|-o \./$o\$" | head -1)
        [ -n "$cmd" ] || { echo "no rule for $o in $tree" >&2; exit 2; }
        echo "cd '$tree/syzgydb_amd/csrc' && ${cmd% -o *} --cuda-device-only -o $out/$o 2>/dev/null"
    done
done > "$tmp/cmds"
xargs -P "$jobs" -I{} sh -c {} < "$tmp/cmds"
status=0
printf '%-26s %-64s %-64s %s\n' object "parent sha256" "new sha256" same
for o in $objs; do
    a=$(sha256sum < "$parent/syzgydb_amd/csrc/$out/$o" | cut -d' ' -f1)
    b=$(sha256sum < "$here/syzgydb_amd/csrc/$out/$o" | cut -d' ' -f1)
    same=yes; [ "$a" = "$b" ] || { same=NO; status=1; }
    printf '%-26s %s %s %s\n' "${o%.o}" "$a" "$b" "$same"
done
exit $status
