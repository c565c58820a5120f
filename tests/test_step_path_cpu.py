"""CPU: resolve_step_path() (csrc/m3g_step_path.h) is the one host function that turns plan options, sizes and topology hints into the
kernel path of a step.  tests/c_abi/m3g_step_path_check.cpp prints it for a table of cases on each side of every threshold; here that
program is built with the host compiler of ROCm under the address and undefined-behaviour sanitizers, run, and its table compared with
what the conditions of the dispatcher and the launchers say (written down from them, case by case)."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

# rev: 0 VALU, 1 node-MLP + edge-MLP pair, 2 fused bf16/f16, 3 persistent fp32, 4 split-tile fp32.  ro (readout): 0 VALU, 1 split, 2 fp32
# chains, 3 fp16 chains.  tail, one digit per block from block 0: 0 separate launches, 1 side-stream overlap, 2 one-launch node +
# three-body candidate, 3 final three-body + geometry.  stress: 0 none, 1 in the force gather, 2 pair virial, 3 reference kernel.
# dp1: 0 fp32 rows, 1 packed, 2 fixed point, 3 fp32 rows by destination.
BASE = dict(pipe=1, fused=1, acts=2, fsave=2, dp1=0, mom=1, long=0, geo_np=1, nsplit=1, fwd=1, rev=4, st=1, ro=1, rsum=1, edef=0, tail="322",
            small=1, gv=1, stress=1)
NO_MOMENTS = dict(mom=0, tail="000")
MANY_ATOMS = dict(rsum=0, edef=1, tail="300", small=0, gv=0, stress=3)   # beyond kFusedSumsMaxAtoms: stand-alone sums, virial kernel forms both
SPLIT_MODE = dict(acts=0, fsave=0, geo_np=0, nsplit=0, fwd=0, rev=2)      # bf16x3 / f16x3: nothing saved, no fp32-only small-system kernels
EXPECT = {
    "default": {},
    "etiles=1536": {},
    "etiles=1537": dict(rev=3),
    "etiles=3072": dict(rev=3),
    "etiles=3073": dict(rev=3, fwd=0),
    "ntiles=128": MANY_ATOMS,
    "ntiles=129": dict(MANY_ATOMS, geo_np=0, nsplit=0, ro=2),
    "N=128": {},
    "N=129": dict(tail="300"),
    "N=1024": dict(tail="300"),
    "N=1025": MANY_ATOMS,
    "S=8": {},
    "S=9": dict(rsum=0, edef=1, gv=0, stress=3),
    "T=24E": {},
    "T=24E+1": dict(long=1),
    "hints=0": NO_MOMENTS,
    "hints_incomplete": NO_MOMENTS,
    "hints_rows=0": NO_MOMENTS,
    "hints_atoms=0": NO_MOMENTS,
    "L=4": NO_MOMENTS,
    "B=0": dict(tail="-", geo_np=0),
    "B=1": dict(tail="3"),
    "E=0": dict(geo_np=0, fwd=0, rev=3, tail="000"),
    "T=0": dict(tail="000"),
    "N=0": dict(geo_np=0, fwd=0, rev=3, tail="000", rsum=0, gv=0, stress=3),
    "forces_off": dict(fsave=0, tail="000", small=0, gv=0, stress=0),
    "stresses_off": dict(gv=0, stress=0),
    "stress_mode=1": dict(gv=0, stress=2),
    "profile": dict(geo_np=0, tail="000"),
    "edge_kernel=0": dict(pipe=0, fused=0, acts=0, fsave=0, geo_np=0, nsplit=0, fwd=0, rev=0, st=0, ro=0, rsum=0, tail="000", gv=0, stress=3),
    "edge_kernel=2": dict(pipe=2, fused=0, acts=0, fsave=0, mom=0, geo_np=0, nsplit=0, fwd=0, rev=0, st=0, ro=0, rsum=0, tail="000", small=0, gv=0,
                          stress=0),   # the any-size path decides for itself: nothing else is resolved
    "rev_kernel=0": dict(fused=0, acts=1, fsave=1, fwd=0, rev=1, tail="000"),
    "precision=1": dict(SPLIT_MODE, dp1=1),
    "precision=2": dict(SPLIT_MODE, dp1=2),
    "save_p1=0": dict(fused=0, acts=0, fsave=0, rev=1, tail="000"),
    "save_p2=0": dict(acts=1, fsave=1, fwd=0, rev=3),
    "dp1_by_dst=1": dict(dp1=3),
    "fuse_node_tb=0": dict(tail="300"),
    "small_launches=0": dict(geo_np=0, nsplit=0, ro=2, rsum=0, tail="022", small=0, gv=0, stress=3),
    "split_tail=0": dict(st=0),
    "split_tail=2": dict(st=2),
    "overlap=1": dict(tail="311"),
    "threebody_moments=0": NO_MOMENTS,
    "legendre_backward=1": NO_MOMENTS,
    "readout_f16=1,precision=2": dict(SPLIT_MODE, dp1=2, ro=3),
    "small_tiles=0": dict(fwd=0, rev=3),
    "stamps": dict(fwd=0, rev=3),
}


def test_resolved_step_path_of_every_threshold_and_option(tmp_path):
    cxx = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin" / "clang++"
    binary = tmp_path / "m3g_step_path_check"
    build = subprocess.run([str(cxx), "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            str(ROOT / "tests" / "c_abi" / "m3g_step_path_check.cpp"), "-o", str(binary)], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    proc = subprocess.run([str(binary)], capture_output=True, text=True, timeout=60)
    assert proc.returncode == 0 and not proc.stderr, proc.stderr[-3000:]
    got = {}
    for line in proc.stdout.splitlines():
        name, *fields = line.split()
        got[name] = {k: (v if k == "tail" else int(v)) for k, v in (f.split("=") for f in fields)}
    assert list(got) == list(EXPECT)
    for name, change in EXPECT.items():
        want = dict(BASE, **change)
        diff = {k: (got[name][k], want[k]) for k in want if got[name][k] != want[k]}
        assert not diff and got[name].keys() == want.keys(), f"{name}: (resolved, expected) {diff}"


# tiles -> {tiles per workgroup: workgroups}, worked out from tiles_for, grid_for_tiles and the TileQueue constructor of
# csrc/m3g_edge_common.h: 84 (32-atom cell: one tile per workgroup, 88 launched), 284 (108 atoms: two each on 142 of 256 workgroups),
# 672 (256 atoms), 2,268 (864 atoms: 9 each, the last workgroup of an XCD's eighth 5, of the last eighth 1), 5,376 (2,048 atoms)
TILE_COUNTS = {84: {1: 84, 0: 4}, 284: {2: 142, 0: 114}, 672: {3: 224, 0: 32}, 2268: {9: 248, 5: 7, 1: 1}, 5376: {21: 256}}


def test_restated_tile_queue_gives_the_kernels_share_per_workgroup():
    """helpers.persistent_tile_counts is what the GPU tests use to assert the regime their input puts k_edge_rev_f32 in (a wave's
    second tile, the split tail): pinned here to the table above, and to the invariants of the queue for every size up to 6,000 tiles."""
    from helpers import persistent_tile_counts, split_tail_runs, wave_takes_a_second_tile

    for tiles, want in TILE_COUNTS.items():
        for n_edges in (16 * tiles - 15, 16 * tiles):   # a part-filled last tile is a tile
            assert dict(persistent_tile_counts(n_edges)) == want, (tiles, n_edges)
    for tiles in list(range(0, 600)) + list(range(600, 6000, 37)):
        counts = persistent_tile_counts(16 * tiles)
        assert sum(c * n for c, n in counts.items()) == tiles            # every tile handed out once
        assert sum(counts.values()) == min(max((tiles + 7) // 8 * 8, 8), 256)
    assert not wave_takes_a_second_tile(persistent_tile_counts(16 * 672)) and wave_takes_a_second_tile(persistent_tile_counts(16 * 2268))
    assert not split_tail_runs(persistent_tile_counts(16 * 284), 1) and split_tail_runs(persistent_tile_counts(16 * 284), 2)
    assert split_tail_runs(persistent_tile_counts(16 * 84), 1) and split_tail_runs(persistent_tile_counts(16 * 2268), 1)
    assert not split_tail_runs(persistent_tile_counts(16 * 672), 2)
