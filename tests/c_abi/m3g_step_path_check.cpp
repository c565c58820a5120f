// Prints the kernel path resolve_step_path() (csrc/m3g_step_path.h) gives for a fixed table of cases, one line each: each side of
// every size threshold, the topology hints, and every option that moves the path.  Host code only (tests/test_step_path_cpu.py
// builds it with the sanitizers of the host compiler and compares the table with expectations written down from the conditions).
#include <cstdio>

#include "../../torch-m3gnet_amd/csrc/m3g_step_path.h"

using namespace m3g;

struct Case {
  Options o;
  ModelDims m{3, 3, 9, 3};
  int64_t N = 32, E = 1000, T = 5000, S = 1;
  int hints = M3G_TOPO_TB_COMPLETE | (64 << 8) | (8 << 16);   // complete lists, windows of 64 rows over 8 atoms
  bool forces = true, stresses = true, profile = false;
};

static void run(const char* name, void (*change)(Case&)) {
  Case c;
  change(c);
  const StepPath p = resolve_step_path(c.o, c.m, c.N, c.E, c.T, c.S, c.hints, c.forces, c.stresses, c.profile);
  char tail[kMaxBlocks + 2] = "-";
  for (int b = 0; b < c.m.B && b < kMaxBlocks; ++b) { tail[b] = (char)('0' + p.tail[b]); tail[b + 1] = 0; }
  printf("%s pipe=%d fused=%d acts=%d fsave=%d dp1=%d mom=%d long=%d geo_np=%d nsplit=%d fwd=%d rev=%d st=%d ro=%d rsum=%d edef=%d tail=%s small=%d gv=%d "
         "stress=%d\n",
         name, p.pipeline, (int)p.fused_rev, p.saved_acts, p.fwd_save, p.dp1, (int)p.moments, (int)p.long_lists, (int)p.geom_with_node_pre,
         (int)p.node_split, (int)p.fwd_split, p.rev_edge, p.split_tail, p.readout, (int)p.readout_sums, (int)p.energy_deferred, tail,
         (int)p.node_rev_small, (int)p.gather_virial, p.stress);
}

int main() {
  run("default", [](Case&) {});
  // 16-edge tiles against small_tiles (1536) and small_tiles_fwd (3072)
  run("etiles=1536", [](Case& c) { c.E = 1536 * 16; });
  run("etiles=1537", [](Case& c) { c.E = 1536 * 16 + 1; });
  run("etiles=3072", [](Case& c) { c.E = 3072 * 16; });
  run("etiles=3073", [](Case& c) { c.E = 3072 * 16 + 1; });
  // 16-atom tiles against split_node_tiles (128)
  run("ntiles=128", [](Case& c) { c.N = 2048; });
  run("ntiles=129", [](Case& c) { c.N = 2049; });
  run("N=128", [](Case& c) { c.N = 128; });     // kNodeTbFusedMaxAtoms
  run("N=129", [](Case& c) { c.N = 129; });
  run("N=1024", [](Case& c) { c.N = 1024; });   // kFusedSumsMaxAtoms
  run("N=1025", [](Case& c) { c.N = 1025; });
  run("S=8", [](Case& c) { c.S = 8; });         // kForceTailMaxStructs
  run("S=9", [](Case& c) { c.S = 9; });
  run("T=24E", [](Case& c) { c.T = 24 * c.E; });
  run("T=24E+1", [](Case& c) { c.T = 24 * c.E + 1; });
  run("hints=0", [](Case& c) { c.hints = 0; });
  run("hints_incomplete", [](Case& c) { c.hints &= ~M3G_TOPO_TB_COMPLETE; });
  run("hints_rows=0", [](Case& c) { c.hints &= ~0xff00; });
  run("hints_atoms=0", [](Case& c) { c.hints &= ~0xff0000; });
  run("L=4", [](Case& c) { c.m = ModelDims{4, 3, 12, 3}; });
  run("B=0", [](Case& c) { c.m.B = 0; });
  run("B=1", [](Case& c) { c.m.B = 1; });
  run("E=0", [](Case& c) { c.E = 0; c.T = 0; });
  run("T=0", [](Case& c) { c.T = 0; });
  run("N=0", [](Case& c) { c.N = 0; c.E = 0; c.T = 0; });
  run("forces_off", [](Case& c) { c.forces = false; c.stresses = false; });
  run("stresses_off", [](Case& c) { c.stresses = false; });
  run("stress_mode=1", [](Case& c) { c.o.stress_mode = 1; });
  run("profile", [](Case& c) { c.profile = true; });
  run("edge_kernel=0", [](Case& c) { c.o.edge_kernel = 0; });
  run("edge_kernel=2", [](Case& c) { c.o.edge_kernel = 2; });
  run("rev_kernel=0", [](Case& c) { c.o.rev_kernel = 0; });
  run("precision=1", [](Case& c) { c.o.precision = 1; });
  run("precision=2", [](Case& c) { c.o.precision = 2; });
  run("save_p1=0", [](Case& c) { c.o.save_p1 = 0; });
  run("save_p2=0", [](Case& c) { c.o.save_p2 = 0; });
  run("dp1_by_dst=1", [](Case& c) { c.o.dp1_by_dst = 1; });
  run("fuse_node_tb=0", [](Case& c) { c.o.fuse_node_tb = 0; });
  run("small_launches=0", [](Case& c) { c.o.small_launches = 0; });
  run("split_tail=0", [](Case& c) { c.o.split_tail = 0; });
  run("split_tail=2", [](Case& c) { c.o.split_tail = 2; });
  run("overlap=1", [](Case& c) { c.o.overlap = 1; });
  run("threebody_moments=0", [](Case& c) { c.o.tb_moments = 0; });
  run("legendre_backward=1", [](Case& c) { c.o.legendre_ref = 1; });
  run("readout_f16=1,precision=2", [](Case& c) { c.o.readout_f16 = 1; c.o.precision = 2; });
  run("small_tiles=0", [](Case& c) { c.o.small_tiles = c.o.small_tiles_fwd = 0; });   // (the setter moves both thresholds)
  run("stamps", [](Case& c) { c.o.stamp_target = 1; });
  return 0;
}
