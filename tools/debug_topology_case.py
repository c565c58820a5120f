"""Case `n` of tests/checkers/fuzz_topology_build.py (same random stream) through the general and the canonical topology build: which
regions of the two buffers differ, and where.  The layout is the library's own (m3g_debug_topology_layout).
Usage: python tools/debug_topology_case.py CASE"""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "torch-m3gnet_amd", ROOT / "tests", ROOT / "tests/checkers"):
    sys.path.insert(0, str(p))
from fuzz_graph_build import random_cell  # noqa: E402
from test_gpu_graph_build import _topology_buffers  # noqa: E402
from topology_reference import REGIONS  # noqa: E402
from torch_m3gnet import _lib  # noqa: E402
from torch_m3gnet.data import MaterialGraphKey as K  # noqa: E402
from torch_m3gnet.data.graph_gpu import batch_from_arrays  # noqa: E402


def layout(N, E, T, S):
    """[(region, byte offset, documented elements, bytes per element)]"""
    off, n, b = (C.c_int64 * 32)(), (C.c_int64 * 32)(), (C.c_int32 * 32)()
    count = C.c_int32()
    _lib.check(_lib.load_library().m3g_debug_topology_layout(N, E, T, S, 32, off, n, b, C.byref(count)))
    assert count.value == len(REGIONS)
    return [(name, int(off[i]), int(n[i]), int(b[i])) for i, name in enumerate(REGIONS)]


def main():
    target = int(sys.argv[1])
    rng = np.random.default_rng(0)
    for c in range(target + 1):
        cutoff = float(rng.uniform(2.5, 9.0))
        tb = float(rng.uniform(0.5, 1.0) * cutoff) if rng.random() < 0.8 else cutoff
        cells = [random_cell(rng) for _ in range(int(rng.integers(1, 7)))]
        if min(abs(np.linalg.det(l)) for l, _ in cells) < 4.0:
            continue
        g = batch_from_arrays([l for l, _ in cells], [p for _, p in cells], [np.full(len(p), 14) for _, p in cells], cutoff, tb, device="cuda")
        if c < target:
            continue
        N, E, T, S = int(g[K.NUM_NODES]), int(g[K.NUM_EDGES]), int(g[K.NUM_TRIPLETS]), len(cells)
        (a, ha, fa), (b, hb, fb), path = _topology_buffers(g)
        print("N E T S", N, E, T, S, "bytes", a.numel())
        for name, off, n, width in layout(N, E, T, S):
            dt = torch.uint8 if width == 1 else torch.int32
            ia, ib = a[off:off + n * width].view(dt), b[off:off + n * width].view(dt)
            if not torch.equal(ia, ib):
                idx = torch.nonzero(ia != ib).flatten()
                print(name, "differs at", idx.numel(), "elements:", idx[:8].tolist(), "general", ia[idx[:8]].tolist(), "canonical", ib[idx[:8]].tolist())
            if name in ("flags", "tb_win", "tb_fast"):
                print(name, "general", ia[:12].tolist(), "canonical", ib[:12].tolist())
        print("hints", hex(ha), hex(hb), "path", path)


if __name__ == "__main__":
    main()
