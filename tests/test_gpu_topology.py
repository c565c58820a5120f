"""Every array of the topology buffer (csrc/m3g_topology.hip) against its host restatement (tests/topology_reference.py), element by
element and for equality: all of it is integer work.

Each case of tests/topology_cases.py goes through every entry point its lists admit -- m3g_topology_build, m3g_topology_hints on
that buffer, m3g_topology_build_hints and, for lists as the library's builders write them, m3g_topology_build_canonical and its
_begin / _end pair -- into a buffer of exactly m3g_topology_bytes, once pre-filled with 0x00 and once with 0xA5: a documented element
that differs between the fills was never written.  The layout comes from m3g_debug_topology_layout.  The buffers a trajectory builds
behind a refill (VerletGraph.update) and inside m3g_md_step are held against the restatement of the lists written there.
Which branch of the general build a case takes (optimistic, sorted again, one-sided second sort, in-edge sort fallback, no triplets)
is INFERRED from its lists (topology_cases.Case.branch, which restates the build's decisions and the 512-edge stage of the mirror
search by hand) and not observed on the device: only the canonical entry points report their path (m3g_topology_debug_last_path).
Times per test: profiles/topology_restatement.txt."""
import ctypes as C

import numpy as np
import pytest
import torch

import topology_cases as tc
import topology_reference as tr

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILLS = (0x00, 0xA5)


def _lib():
    from torch_m3gnet import _lib as lib_module

    return lib_module, lib_module.load_library()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _regions(buf: torch.Tensor, N, E, T, S) -> dict:
    """{region: its documented elements} of a topology buffer, by the library's own layout."""
    mod, lib = _lib()
    off, n, b = (C.c_int64 * 32)(), (C.c_int64 * 32)(), (C.c_int32 * 32)()
    count = C.c_int32()
    mod.check(lib.m3g_debug_topology_layout(N, E, T, S, 32, off, n, b, C.byref(count)))
    assert count.value == len(tr.REGIONS)
    data = C.c_size_t()
    mod.check(lib.m3g_topology_data_bytes(N, E, T, S, C.byref(data)))
    host = buf[: data.value].cpu().numpy()
    out = {}
    for i, name in enumerate(tr.REGIONS):
        raw = host[off[i]: off[i] + n[i] * b[i]]
        out[name] = raw.copy() if b[i] == 1 else raw.view(np.int32).copy()
    return out


def _scalars(buf, N, E, T, S):
    mod, lib = _lib()
    count, status = C.c_int64(-1), C.c_int32(-1)
    mod.check(lib.m3g_topology_active_edges(N, E, T, S, _ptr(buf), C.byref(count), _stream()))
    mod.check(lib.m3g_topology_status(N, E, T, S, _ptr(buf), C.byref(status), _stream()))
    return int(count.value), int(status.value)


class _Device:
    """A case's index tensors on the device and fresh buffers of exactly m3g_topology_bytes."""

    def __init__(self, c: tc.Case):
        mod, lib = _lib()
        self.c = c
        self.sizes = (c.N, c.E, c.T, c.S)
        self.ei = torch.tensor(c.edge_index, device=DEV)
        self.tei = torch.tensor(c.triplet_edge_index, device=DEV)
        self.batch = torch.tensor(c.batch, device=DEV)
        nbytes = C.c_size_t()
        mod.check(lib.m3g_topology_bytes(*self.sizes, C.byref(nbytes)))
        self.nbytes = nbytes.value
        self.verdict = torch.zeros(16, dtype=torch.int32).pin_memory()

    def buffer(self, fill):
        return torch.full((self.nbytes,), fill, dtype=torch.uint8, device=DEV)

    def lists(self):
        return _ptr(self.ei), _ptr(self.tei), _ptr(self.batch)

    def run(self, entry, fill):
        """[(entry point name, regions, hints word or None, host_flags, A, status, path or None)]: "build" yields the buffer after
        m3g_topology_build and again after m3g_topology_hints on it."""
        mod, lib = _lib()
        buf = self.buffer(fill)
        flags, hints, path = (C.c_int32 * 1)(-1), C.c_int32(-1), C.c_int32(-1)
        args = (*self.sizes, *self.lists(), _ptr(buf), self.nbytes)
        out = []

        def snapshot(name, word, with_path=False):
            torch.cuda.synchronize()
            if with_path:
                mod.check(lib.m3g_topology_debug_last_path(C.byref(path)))
            out.append((name, _regions(buf, *self.sizes), word, int(flags[0]), *_scalars(buf, *self.sizes), int(path.value) if with_path else None))

        if entry == "build":
            mod.check(lib.m3g_topology_build(*args, flags, _stream()))
            snapshot("m3g_topology_build", None)
            mod.check(lib.m3g_topology_hints(*self.sizes, _ptr(buf), C.byref(hints), _stream()))
            snapshot("m3g_topology_hints after m3g_topology_build", int(hints.value))
        elif entry == "build_hints":
            mod.check(lib.m3g_topology_build_hints(*args, flags, C.byref(hints), _stream()))
            snapshot("m3g_topology_build_hints", int(hints.value))
        elif entry == "canonical":
            mod.check(lib.m3g_topology_build_canonical(*args, flags, C.byref(hints), _stream()))
            snapshot("m3g_topology_build_canonical", int(hints.value), with_path=True)
        elif entry == "canonical_begin_end":
            self.verdict.zero_()
            verdict = C.c_void_p(self.verdict.data_ptr())
            mod.check(lib.m3g_topology_build_canonical_begin(*args, verdict, _stream()))
            mod.check(lib.m3g_topology_build_canonical_end(*args, verdict, flags, C.byref(hints), _stream()))
            snapshot("m3g_topology_build_canonical_begin / _end", int(hints.value), with_path=True)
        else:
            raise KeyError(entry)
        return out


def _hold(case_name, entry_name, got, ref):
    bad = tr.first_mismatch(got, ref)
    if bad is not None:
        region, i, dev, want = bad
        raise AssertionError(f"case '{case_name}', {entry_name}: {region}[{i}] is {dev} on the device, {want} in the restatement")


def _same_under_both_fills(case_name, entry_name, a, b, ref):
    # (struct_ptr is compared at its whole length also where the restatement leaves it unspecified: every build writes it -- the
    #  lower bounds of `batch` as it is -- and only what it MEANS is undefined for an unsorted batch)
    for region in tr.REGIONS:
        n = len(ref[region]) if ref[region] is not None else len(a[region])
        diff = np.nonzero(a[region][:n] != b[region][:n])[0]
        if len(diff):
            i = int(diff[0])
            raise AssertionError(f"case '{case_name}', {entry_name}: {region}[{i}] is never written -- {int(a[region][i])} in a buffer "
                                 f"pre-filled with 0x00, {int(b[region][i])} with 0xA5")


@pytest.mark.parametrize("name", tc.NAMES)
def test_every_entry_point_writes_the_restatement(name):
    c, ref = tc.case(name), tc.reference(name)
    bare = tr.without_certificate(ref)
    dev = _Device(c)
    entries = ("build", "build_hints") + (("canonical", "canonical_begin_end") if c.canonical else ())
    for entry in entries:
        by_fill = [dev.run(entry, fill) for fill in FILLS]
        for results in by_fill:
            for entry_name, got, word, host_flags, n_act, status, path in results:
                want = bare if word is None else ref
                _hold(name, entry_name, got, want)
                assert word is None or word == ref["hints"], (name, entry_name, hex(word), hex(ref["hints"]))
                assert (host_flags, n_act, status) == (0, ref["A"], 0), (name, entry_name, host_flags, n_act, status, ref["A"])
                if path is not None:
                    assert path == (1 if c.fast_build_applies else 0), (name, entry_name, path)
        for (entry_name, a, *_), (_, b, *_) in zip(*by_fill):
            _same_under_both_fills(name, entry_name, a, b, ref)


# ------------------------------------------------------------------ the buffers a trajectory builds
def _trajectory():
    from torch_m3gnet.data.synthetic import fcc_cu_arrays

    lat, pos, z = fcc_cu_arrays(2, 2, 2, jitter=0.05, seed=3)
    drift = np.random.default_rng(4).normal(0.0, 1.0, pos.shape)
    return lat, z, [pos, pos + 0.05 * drift]


def _graph_lists(N, S, ei, tei, batch):
    return tr.restate(N, S, ei.cpu().numpy(), tei.cpu().numpy(), batch.cpu().numpy())


def test_the_buffer_behind_a_verlet_refill():
    """VerletGraph queues the canonical build behind the lists it has just written (m3g_topology_build_canonical_begin, ended by
    `finish`): the buffer against the restatement of those lists, at the first fill and at a refill."""
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.md import VerletGraph

    lat, z, frames = _trajectory()
    vg = VerletGraph([lat], [z], 5.0, 4.0, skin=0.5, device=DEV)
    for step, pos in enumerate(frames):
        g = vg.update(torch.tensor(pos, device=DEV), force="refill" if step else None)
        topo = g["_m3g_topology"][1].finish()
        torch.cuda.synchronize()
        ref = _graph_lists(vg.N, vg.S, g[K.EDGE_INDEX], g[K.TRIPLET_EDGE_INDEX], g[K.BATCH])
        sizes = (vg.N, int(g[K.NUM_EDGES]), int(g[K.NUM_TRIPLETS]), vg.S)
        assert sizes[2] > 0 and ref["hints"] != 0
        _hold(f"trajectory frame {step}", "VerletGraph.update", _regions(topo.buf, *sizes), ref)
        assert topo.query_hints() == ref["hints"] and _scalars(topo.buf, *sizes) == (ref["A"], 0)
    assert vg.stats["refill"] == 2


def test_the_buffer_inside_md_step():
    """m3g_md_step builds the topology on the C side, in a buffer of the candidates' capacity carved for the step's own counts:
    held against the restatement of the lists the step ran on (VerletGraph.step_lists)."""
    from torch_m3gnet.data import MaterialGraphKey as K
    from torch_m3gnet.data.md import VerletGraph
    from torch_m3gnet.model.build import build_model

    torch.manual_seed(0)
    model = build_model(5.0, 4.0, 3, 3, 95, 64, 3).to(DEV)
    lat, z, frames = _trajectory()
    vg = VerletGraph([lat], [z], 5.0, 4.0, skin=0.5, device=DEV)
    for step, pos in enumerate(frames):
        out = vg.step(model, torch.tensor(pos, device=DEV), force="refill" if step else None)
        torch.cuda.synchronize()
        assert vg._lists_owner == "c" and bool(torch.isfinite(out[K.FORCES]).all())
        lists = vg.step_lists()
        n_e, n_t = vg._step_sizes
        ref = _graph_lists(vg.N, vg.S, lists[K.EDGE_INDEX], lists[K.TRIPLET_EDGE_INDEX], vg.batch)
        assert n_t > 0 and ref["hints"] != 0
        _hold(f"trajectory frame {step}", "m3g_md_step", _regions(vg._md_buffers["topo"], vg.N, n_e, n_t, vg.S), ref)
        assert _scalars(vg._md_buffers["topo"], vg.N, n_e, n_t, vg.S) == (ref["A"], 0)
