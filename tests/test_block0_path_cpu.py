"""CPU: StepPath::block0 of resolve_step_path() (csrc/m3g_step_path.h) -- whether block 0's node rows come from its node kernel (0),
from the plan's per-species tables as the second workgroup role of the geometry launch (1), or from the tables in a launch of their
own (2: stage profiler on, or no edge and so no geometry launch).  tests/c_abi/m3g_block0_path_check.cpp prints it for a table of
cases; built here with the host compiler of ROCm under the address and undefined-behaviour sanitizers and compared with what the
conditions say.  geom_with_node_pre keeps the value it had before the field existed (tests/test_step_path_cpu.py holds the rest)."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent

# name -> (block0, geo_np)
EXPECT = {
    "default": (1, 1),
    "ntiles=129": (1, 0),
    "N=10000": (1, 0),
    "forces_off": (1, 1),
    "precision=1": (1, 0),            # every precision has its own tables
    "precision=2": (1, 0),
    "small_launches=0": (1, 0),
    "profile": (2, 0),
    "profile,N=10000": (2, 0),
    "E=0": (2, 0),
    "N=0": (0, 0),                    # no atom: no rows
    "B=0": (0, 0),                    # no block: k_embed_nodes_only forms x^0
    "species_tables=0": (0, 1),
    "species_tables=0,N=10000": (0, 0),
    "species_tables=0,profile": (0, 0),
    "edge_kernel=0": (0, 0),          # the vector-ALU baseline has its own embedding kernel
    "edge_kernel=2": (0, 0),          # the any-size path resolves nothing here
}


def test_block0_of_the_resolved_step_path(tmp_path):
    cxx = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "llvm" / "bin" / "clang++"
    binary = tmp_path / "m3g_block0_path_check"
    build = subprocess.run([str(cxx), "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            str(ROOT / "tests" / "c_abi" / "m3g_block0_path_check.cpp"), "-o", str(binary)], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    proc = subprocess.run([str(binary)], capture_output=True, text=True, timeout=60)
    assert proc.returncode == 0 and not proc.stderr, proc.stderr[-3000:]
    got = {}
    for line in proc.stdout.splitlines():
        name, *fields = line.split()
        values = dict(f.split("=") for f in fields)
        got[name] = (int(values["block0"]), int(values["geo_np"]))
    assert got == EXPECT, {k: (got.get(k), v) for k, v in EXPECT.items() if got.get(k) != v}
