// Prints StepPath::block0 (csrc/m3g_step_path.h: how block 0's node rows are formed) beside geom_with_node_pre for a table of cases,
// one line each.  Host code only (tests/test_block0_path_cpu.py builds it with the sanitizers of the host compiler).
#include <cstdio>

#include "../../torch-m3gnet_amd/csrc/m3g_step_path.h"

using namespace m3g;

struct Case {
  Options o;
  ModelDims m{3, 3, 9, 3};
  int64_t N = 32, E = 1000, T = 5000, S = 1;
  int hints = M3G_TOPO_TB_COMPLETE | (64 << 8) | (8 << 16);
  bool forces = true, profile = false;
};

static void run(const char* name, void (*change)(Case&)) {
  Case c;
  change(c);
  const StepPath p = resolve_step_path(c.o, c.m, c.N, c.E, c.T, c.S, c.hints, c.forces, c.forces, c.profile);
  printf("%s block0=%d geo_np=%d\n", name, p.block0, (int)p.geom_with_node_pre);
}

int main() {
  run("default", [](Case&) {});
  run("ntiles=129", [](Case& c) { c.N = 2049; });
  run("N=10000", [](Case& c) { c.N = 10000; c.E = 420000; c.T = 2000000; });
  run("forces_off", [](Case& c) { c.forces = false; });
  run("precision=1", [](Case& c) { c.o.precision = 1; });
  run("precision=2", [](Case& c) { c.o.precision = 2; });
  run("small_launches=0", [](Case& c) { c.o.small_launches = 0; });
  run("profile", [](Case& c) { c.profile = true; });
  run("profile,N=10000", [](Case& c) { c.profile = true; c.N = 10000; c.E = 420000; });
  run("E=0", [](Case& c) { c.E = 0; c.T = 0; });
  run("N=0", [](Case& c) { c.N = 0; c.E = 0; c.T = 0; });
  run("B=0", [](Case& c) { c.m.B = 0; });
  run("species_tables=0", [](Case& c) { c.o.species_tables = 0; });
  run("species_tables=0,N=10000", [](Case& c) { c.o.species_tables = 0; c.N = 10000; c.E = 420000; });
  run("species_tables=0,profile", [](Case& c) { c.o.species_tables = 0; c.profile = true; });
  run("edge_kernel=0", [](Case& c) { c.o.edge_kernel = 0; });
  run("edge_kernel=2", [](Case& c) { c.o.edge_kernel = 2; });
  return 0;
}
