#!/bin/bash
# usage: SRC=<dir> [FILES="m3g_node ..."] tools/build_variant.sh <name> [extra hipcc flags...]   -> torch-m3gnet_amd/lib/variants/<name>.so
# Builds the kernels of ANOTHER checkout into a library that tools/bench_variants.sh can time next to the built one on the same
# box -- how a change is compared with its parent commit.  SRC = the directory with that checkout's csrc/*.hip,*.h, e.g. a
# `git worktree` of the parent (default: csrc, this tree's own).  FILES names the sources taken from SRC (default: the MFMA edge
# kernels m3g_edge_mfma.hip and m3g_edge_rev_f32.hip); every other object comes from this tree's build/.  Prints the register
# and spill use of the three main edge kernels.
set -e
cd "$(dirname "$0")/../torch-m3gnet_amd"
name=$1; shift
src=${SRC:-csrc}
mkdir -p lib/variants
files=${FILES:-"m3g_edge_mfma m3g_edge_rev_f32"}
for f in $files; do
  /opt/rocm/bin/hipcc -O3 -std=c++20 --offload-arch=gfx950 -fPIC -I../include "$@" -Rpass-analysis=kernel-resource-usage -c $src/$f.hip -o /tmp/${f}_$name.o 2>&1 | grep -A8 "k_edge_rev_fusedILi3ELb1\|k_edge_block_mfmaILi3ELb0ELb0\|k_edge_rev_f32ILi3ELb1" | grep -E "Name|VGPRs:|ScratchSize" | sed "s/.*remark: /  /" | cut -c1-100 &
done
wait
objs=""; skip="NONE"
for f in $files; do objs="$objs /tmp/${f}_$name.o"; skip="$skip\|$f.o"; done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o lib/variants/$name.so $objs $(ls build/*.o | grep -v "$skip")
