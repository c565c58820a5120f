"""The inputs of tests/test_gpu_rnemd.py: a batch of 7, 257 and 64 atoms, built so that every edge of the exchange occurs, and the
checks that it does (run on the restatement alone by tests/test_rnemd_cpu.py, and on the device's answers by the GPU test)."""
import numpy as np

import rnemd_reference as rr

SIZES = [7, 257, 64]
KIND = {"heat": rr.HEAT, "momentum": rr.MOMENTUM}
AXIS, FLOW = 2, 0
# (kind, n_slabs, n_swaps, mixed masses, active mask)
CASES = [("heat", 2, 1, False, False), ("heat", 6, 3, True, True), ("heat", 64, 8, False, True), ("heat", 6, 8, False, False),
         ("momentum", 2, 3, False, True), ("momentum", 6, 8, True, False), ("momentum", 64, 1, True, True), ("momentum", 6, 3, False, False)]
CU = 63.546


def structures(kind: str, mixed: bool, cold_c: bool = False) -> list:
    """[[lattice, positions, masses, velocities, active]] of the three structures.  Fractional coordinates along the slab normal are
    chosen, the Cartesian positions follow; the rows named below sit well inside their slab for 2, 6 and 64 slabs alike."""
    rng = np.random.default_rng(11)
    big, low = 5e-2, -5e-2
    quiet = np.zeros(3) if kind == "heat" else np.full(3, low)   # the coldest row (heat) / the slowest along +flow (momentum)
    out = []
    # A, 7 atoms, triclinic: two rows in slab 0 of six (fewer than 3 or 8 swaps), none in slab 32 of 64 (an empty middle slab)
    lat = np.array([[5.0, 0.4, -0.3], [0.2, 6.0, 0.5], [-0.6, 0.3, 9.0]])
    fz = np.array([0.01, 0.05, 0.3, 0.52, 0.55, 0.8, 0.95]) + np.array([0, -2, 1, 2, -1, 0, 1])
    frac = np.column_stack([rng.uniform(-2, 3, 7), rng.uniform(-2, 3, 7), fz])
    v = rng.normal(0, 1e-2, (7, 3))
    v[:2], v[3:5] = 5.0 * np.abs(v[:2]), -0.02 * np.abs(v[3:5])   # slab 0 ahead of the middle slab in both kinds, whatever the masses
    out.append([lat, frac @ lat, None, v, np.ones(7, bool)])
    # B, 257 atoms, triclinic: row 256 (a chunk of its own) is the best candidate of slab 0; rows 10, 20, 30 of slab 0 and rows 40, 50
    # of the middle slab are duplicates (ties go to the lower row); row 10 is masked out where the case asks for a mask
    lat = np.array([[7.0, 0.3, 0.1], [0.2, 8.0, -0.4], [0.5, 0.1, 30.0]])
    frac = rng.uniform(-2, 3, (257, 3))
    v = rng.normal(0, 1e-2, (257, 3))
    frac[[10, 20, 30], 2] = 0.006 + np.array([1, -2, 0])
    frac[256, 2] = 0.004 - 1
    frac[[40, 50], 2] = 0.51 + np.array([2, -1])
    v[[10, 20, 30]] = big
    v[256] = 1.5 * big
    v[[40, 50]] = quiet
    active = np.ones(257, bool)
    active[[10, 77, 200]] = False
    out.append([lat, frac @ lat, None, v, active])
    # C, 64 atoms, a diagonal power-of-two cell: f = (i % 32) / 32 exactly (on the planes of 64 slabs; rows 0 and 16 on those of 2), row 63
    # at f = -1e-17, which wraps to exactly 1.0: the last slab
    lat = np.diag([4.0, 4.0, 16.0])
    pos = np.column_stack([rng.uniform(-8, 12, 64), rng.uniform(-8, 12, 64), (np.arange(64) % 32) * 0.5 + 16.0 * rng.integers(-2, 3, 64)])
    pos[63, 2] = -1e-17 * 16.0
    v = rng.normal(0, 1e-2, (64, 3))
    if cold_c:   # slab 0 of two colder (slower) than slab 1 in every pair: key0 <= keyMid, nothing is exchanged
        upper = ((np.arange(64) % 32) >= 16) | (np.arange(64) == 63)
        v[~upper] = quiet
        v[upper] = big
    out.append([lat, pos, None, v, np.ones(64, bool)])
    for st in out:
        n = len(st[1])
        st[2] = rng.choice([26.9815, CU, 196.967], n) if mixed else np.full(n, CU)
    out[1][2][[10, 20, 30, 40, 50, 256]] = CU   # the named rows keep one mass: the duplicates tie in both kinds, row 256 stays ahead
    return out


def parts_of(case, ids=(0, 1, 2), cold_c=False) -> list:
    kind, _, _, mixed, masked = case
    parts = [structures(kind, mixed, cold_c)[g] for g in ids]
    if not masked:
        for p in parts:
            p[4] = np.ones(len(p[1]), bool)
    return parts


def references(case, parts) -> list:
    kind, n_slabs, n_swaps, _, _ = case
    return [rr.RnemdReference(p[0], p[2], KIND[kind], AXIS, n_slabs, n_swaps, FLOW, p[4]) for p in parts]


def check_construction(case, refs, first_pairs, calls: int) -> None:
    """The batch holds what the module says, given the three references after `calls` swapping and sampling calls and the pairs
    [3, n_swaps, 2] of the first one."""
    _, n_slabs, n_swaps, _, masked = case
    ra, rb, rc = refs
    assert rb.n_exchanged > 0 and rb.transferred > 0 and rc.n_exchanged > 0
    assert [r.count.sum() for r in refs] == [calls * n for n in SIZES]
    # B: the one-row second chunk holds the best candidate of slab 0; then the duplicates in row order (row 10 only where active)
    want = [256] + ([20, 30] if masked else [10, 20, 30])
    k = min(n_swaps, len(want))
    assert first_pairs[1][:k, 0].tolist() == want[:k], first_pairs[1]
    assert first_pairs[1][0, 1] == 40 and (n_swaps == 1 or first_pairs[1][1, 1] == 50)
    if n_slabs == 6:    # A: fewer rows in slab 0 than swaps
        assert ra.count[0] == calls * 2 and (first_pairs[0][2:] == -1).all() and ra.n_exchanged > 0
    if n_slabs == 64:   # A: no row in the middle slab, nothing is exchanged; C: rows on the slab planes, row 63 (f = -1e-17) in the last slab
        assert ra.n_exchanged == 0 and ra.count[32] == 0
        want = np.zeros(64, dtype=np.int64)
        want[0:62:2], want[62], want[63] = 2, 1, 1
        assert np.array_equal(rc.count, calls * want), rc.count
