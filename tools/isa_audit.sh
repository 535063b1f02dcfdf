#!/bin/bash
# What the compiler made of the kernels: per kernel of every .hip file, registers / scratch, ds_bpermute count and the number of
# "one load, one wait" pairs (a global load followed by s_waitcnt vmcnt(0) with no other load between: a guarded load inside an
# unrolled loop is issued and waited for in every turn).  Runs here (hipcc cross-compiles; no GPU):
#   bash tools/isa_audit.sh [min_pairs]        -> one line per kernel with >= min_pairs such pairs (default 6) or any ds_bpermute
#   bash tools/isa_audit.sh --stats [csrc_dir [hipcc flags ...]]
#       -> one line per kernel, sorted by name: vgpr_count, sgpr_count, private_segment_fixed_size (scratch),
#          group_segment_fixed_size (LDS) and the instruction count.  Made to be diffed: run it over the csrc directory of a
#          checkout of the parent commit and over this one (`diff <(... --stats parent/kmerseek_amd/csrc) <(... --stats)`);
#          extra flags (-DSK_LB_WAVES=2 ...) compile a diagnostic variant.  KEEP_ASM=dir keeps the assembly there.
R=$(cd "$(dirname "$0")/.." && pwd)
STATS=0
if [ "$1" = "--stats" ]; then STATS=1; shift; fi
SRC=$R/kmerseek_amd/csrc
MIN=6
if [ $STATS = 1 ]; then
  if [ -n "$1" ]; then SRC=$1; shift; fi
else
  MIN=${1:-6}; set --
fi
T=${KEEP_ASM:-$(mktemp -d)}
mkdir -p $T
for f in $SRC/*.hip; do
  b=$(basename $f .hip)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 "$@" -S --cuda-device-only -o $T/$b.s $f 2>/dev/null || { echo "$b: compile failed"; continue; }
  if [ $STATS = 1 ]; then
    # instructions are counted between a kernel's label and its .Lfunc_end; the figures come from the metadata at the file's end
    awk -v F=$b '
      /^_Z.*:/ { name=$1; sub(/:$/, "", name); n=0; next }
      /^\t[a-z]/ { n++ }
      /^\.Lfunc_end/ { insts[name]=n }
      /^    \.group_segment_fixed_size:/ { lds=$2 }
      /^    \.name:/ { kn=$2 }
      /^    \.private_segment_fixed_size:/ { scr=$2 }
      /^    \.sgpr_count:/ { sg=$2 }
      /^    \.vgpr_count:/ { printf "%-10s vgpr %3d  sgpr %3d  scratch %4d  lds %6d  insts %6d  %s\n", F, $2, sg, scr, lds, insts[kn], kn }
    ' $T/$b.s | { command -v c++filt >/dev/null && c++filt || cat; } | sort -k 12
    continue
  fi
  awk -v F=$b -v MIN=$MIN '
    /^_Z.*:/ && !/^\.L/ { name=$1; sub(/:$/, "", name); serial=0; pend=0; bp=0 }
    /^\tglobal_load|^\tbuffer_load|^\tflat_load/ { pend = pend ? 2 : 1 }
    /s_waitcnt vmcnt\(0\)/ { if (pend == 1) serial++; pend = 0 }
    /ds_bpermute|ds_permute/ { bp++ }
    /^\.Lfunc_end/ { if (serial >= MIN || bp > 0) printf "%-10s %-70.70s load-wait pairs %3d  ds_bpermute %3d\n", F, name, serial, bp }
  ' $T/$b.s
  grep -E "\.(num_vgpr|private_seg_size)," $T/$b.s | awk -v F=$b '/private_seg_size/ { n=$2; v=$3; if (v+0 > 0) { sub(/\.private_seg_size,/, "", n); printf "%-10s %-70.70s SCRATCH %s bytes\n", F, n, v } }'
done
[ -n "$KEEP_ASM" ] || rm -rf $T
