"""The host-side launch planning of the per-layer kernels -- nflows_amd/csrc/launch_plan.hpp: `plan_sample_tile`,
`sample_rows`, `aligned_tile`, `full_rows`, `plan_element_tile`, `persistent_grid` -- compiled for the HOST from the
product's source at test time, behind a shim that lays out LDS the way each launcher's callable does.  Every result is
held, exactly, to the arithmetic the launchers carried in line before the planner existed, written out below in Python
launcher by launcher: K1 forward (rqs.hip), K1 backward (rqs_bwd.hip), K2 and K4 (misc.hip), K6 (rqs_shared.hip), K5
(rqs.hip), both K9 launchers (splines_lq.hip) and searchsorted (misc.hip).  CPU only."""
import ctypes

import pytest

import launch_plan_shim

KB, KW = 256, 64   # kBlock, kWave
LDS64 = 64 * 1024
D_AXIS = list(range(1, 65)) + [100, 128, 512, 1024, 4096, 6000, 65535, 65536]
K_AXIS = [1, 4, 8, 10, 16, 32]
CUS = [1, 256, 304]


def ru4(n):
    return (n + 3) & ~3


def dt_axis(D):
    return sorted({0, 1, D // 2, D - 1, D})


def batch_axis(R):
    return sorted({0, 1, max(R - 1, 0), R, R + 1, 65536, 262144, 2 ** 31 + 5})


def bins_axis():
    for K in K_AXIS:
        yield K, 3 * K - 1    # linear tails
        yield K, 3 * K + 1    # tails=None


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return launch_plan_shim.build(str(tmp_path_factory.mktemp("launch_plan_host")))


# ---- the launchers' arithmetic as it stood in line (one function per launcher; None = NFA_ERR_UNSUPPORTED) ---------------
def first_rows(lanes, dt, D, batch):
    R = lanes // dt if dt > 0 else lanes // (D if D < lanes else lanes)
    if R < 1:
        R = 1
    if R > batch:
        R = batch
    return R


def old_k1(D, dt, P, batch, backward, hits):
    """nfa_rqs_coupling_f32 / nfa_rqs_coupling_backward_f32: (R, C, lds, offsets)"""
    R = first_rows(KB, dt, D, batch)
    C = 0

    def lds_floats(r):
        chunk_items = C if C > 0 else r * dt
        if backward:
            o = ru4(chunk_items * P) + 8
            off = [o]
            o += ru4(r * D) + 4
            off.append(o)
            o += ru4(r * D) + 4
            off.append(o)
            o += ru4(r * D) + 4
            off.append(o)
        else:
            o = ru4(chunk_items * P) + 4
            off = [o]
            o += ru4(r * D) + 4
            off.append(o)
            o += ru4(r * D) + 4
            off.append(o)
            o += ru4(KB if C > 0 else (r * dt if r * dt > KB // KW else KB // KW))
            off.append(o)
        o += dt + 2 * D + (D + 3) // 4
        return o, off

    while R > 1 and lds_floats(R)[0] * 4 > LDS64:
        R >>= 1
        hits.add("halved")
    if R == 1 and lds_floats(1)[0] * 4 > LDS64:
        if backward:
            fixed = (3 * (ru4(D) + 4) + dt + 2 * D + (D + 3) // 4 + 16) * 4
        else:
            fixed = (2 * (ru4(D) + 4) + KB + dt + 2 * D + (D + 3) // 4 + 8) * 4
        if fixed + KB * P * 4 > LDS64:
            hits.add("unsupported: no room for a chunk")
            return None
        C = (LDS64 - fixed) // (P * 4)
        C = (C // KB) * KB
        if C >= dt:
            C = 0
    floats, off = lds_floats(R)
    lds = floats * 4
    if R * dt >= 65536:
        hits.add("R*dt >= 65536")
    if R * D >= 65536:
        hits.add("R*D >= 65536")
    if lds > LDS64 or R * dt >= 65536 or R * D >= 65536:
        hits.add("unsupported: tile")
        return None
    if C > 0:
        hits.add("chunked")
    return R, C, lds, off


def old_k2(D, dt, pcols, given, batch, hits):
    """nfa_affine_coupling_f32"""
    R = first_rows(KB, dt, D, batch)

    def lds_floats(r):
        o = ru4(r * pcols) + 4
        off = [o]
        o += ru4(r * dt) + 4 if given else 0
        off.append(o)
        o += ru4(r * D) + 4
        off.append(o)
        o += ru4(r * D) + 4
        off.append(o)
        o += ru4(r * dt)
        off.append(o)
        o += dt + 2 * D + (D + 3) // 4
        return o, off

    while R > 1 and lds_floats(R)[0] * 4 > LDS64:
        R >>= 1
        hits.add("halved")
    floats, off = lds_floats(R)
    if floats * 4 > LDS64 or R * D >= 65536:
        hits.add("unsupported: tile")
        return None
    return R, 0, floats * 4, off


def old_k6(F, K, nd, batch, hits):
    """nfa_rqs_shared_f32"""
    tab = F * 3 * (K + 1)
    R = (4 * KB) // F
    if R < 1:
        R = 1
    if R > batch:
        R = batch

    def lds_floats(r):
        o = (tab + 3) & ~3
        off = [o]
        o += ru4(r * F) + 8
        off.append(o)
        o += ru4(r * F)
        off.append(o)
        o += ru4(F * (2 * K + nd))
        return o, off

    while R > 1 and lds_floats(R)[0] * 4 > LDS64:
        R >>= 1
        hits.add("halved")
    floats, off = lds_floats(R)
    if floats * 4 > LDS64 or R * F >= 65536:
        hits.add("unsupported: tile")
        return None
    return R, 0, floats * 4, off


def old_element_tile(floor, nbytes, hits):
    """`int T = kBlock; while (T > floor && bytes(T) > 64 KB) T >>= 1; if (bytes(T) > 64 KB) unsupported`"""
    T = KB
    while T > floor and nbytes(T) > LDS64:
        T >>= 1
        hits.add("halved")
    if nbytes(T) > LDS64:
        hits.add("unsupported: floor" if T == floor else "unsupported")
        return 0
    return T


def old_grid(cus, lds, cap, tiles):
    """`per_cu = clamp(160 KB / (lds + 256), 1, cap); g = min(cus * per_cu, tiles)`"""
    per_cu = (160 * 1024) // (lds + 256)
    if per_cu > cap:
        per_cu = cap
    if per_cu < 1:
        per_cu = 1
    g = cus * per_cu
    return (tiles if g > tiles else g), per_cu


def check_tile(got, want, noffsets, what):
    if want is None:
        assert got[0] == 0, what
        return
    R, C, lds, off = want
    assert got[0] == 1 and got[1] == R and got[2] == C and got[3] == lds and list(got[4:4 + noffsets]) == off, (what, list(got), want)


def test_sample_tiles_of_k1_forward_and_backward(lib):
    out = (ctypes.c_int64 * 12)()
    hits = {False: set(), True: set()}
    for D in D_AXIS:
        for dt in dt_axis(D):
            for K, P in bins_axis():
                for batch in batch_axis(first_rows(KB, dt, D, 2 ** 40)):
                    for backward, fn in ((False, lib.k1_forward), (True, lib.k1_backward)):
                        want = old_k1(D, dt, P, batch, backward, hits[backward])
                        fn(D, dt, P, batch, out)
                        check_tile(out, want, 4, (D, dt, K, P, batch, backward))
                        if want is None or batch == 0:
                            continue
                        R, C, lds, _ = want
                        # the layouts the pipelined kernels take (both launchers tested the same six conditions)
                        was_aligned = dt > 0 and (dt * P) % 4 == 0 and D % 4 == 0 and R * dt <= KB and R * D <= 2 * KB and R <= batch
                        assert bool(lib.aligned(dt, D, P, R, batch)) == was_aligned
                        if was_aligned:
                            hits[backward].add("aligned")
                        full = (batch // R) * R
                        assert lib.rows_full(batch, R) == full
                        if 0 < full < batch:
                            hits[backward].add("leftover rows")
                        tiles = (batch + R - 1) // R
                        for cus in CUS:
                            g, per_cu = old_grid(cus, lds, 6 if backward else 8, tiles)
                            assert lib.grid_lds(cus, lds, 6 if backward else 8, tiles) == g
                            # the pipelined kernels: `gp = min(cus * min(per_cu, pipe_blocks), full_rows / R)`
                            for pipe_blocks in ((3,) if backward else (6, 4)):
                                gp = cus * (pipe_blocks if per_cu > pipe_blocks else per_cu)
                                if gp > full // R:
                                    gp = full // R
                                assert lib.grid_lds(cus, lds, pipe_blocks, full // R) == gp
                        # whole wave tiles of 64 / d_t rows: `(batch >> (6 - ctz(dt))) << (6 - ctz(dt))`
                        if not backward and 4 <= dt <= 64 and dt & (dt - 1) == 0:
                            shift = 6 - (dt.bit_length() - 1)
                            assert lib.rows_full(batch, 64 // dt) == (batch >> shift) << shift
                            hits[backward].add("wave tiles")
    # (R * d_t >= 65536 and R * D >= 65536 cannot come true behind K1's own layouts: two images of R * D floats within 64 KB
    #  keep R * D <= 8192, and a sample of 65536 features has no room for a chunk -- the next test reaches both)
    for backward in (False, True):
        need = {"halved", "chunked", "unsupported: no room for a chunk", "unsupported: tile", "aligned", "leftover rows"} | \
               (set() if backward else {"wave tiles"})
        assert need <= hits[backward], (backward, need - hits[backward])


def test_item_count_limits_decide_where_lds_does_not(lib):
    """R * d_t >= 65536 and R * D >= 65536 as the DECIDING condition: one float per sample under a 1 GiB budget, the
    launchers' test `lds > budget || R * dt >= 65536 || R * D >= 65536` behind the same first guess and halving"""
    out = (ctypes.c_int64 * 12)()
    hits = set()
    for lanes in (KB, 4 * KB, 1 << 20):
        for D in D_AXIS:
            for dt in dt_axis(D):
                for batch in batch_axis(first_rows(lanes, dt, D, 2 ** 40)):
                    R = first_rows(lanes, dt, D, batch)
                    while R > 1 and R * 4 > 1 << 30:
                        R >>= 1
                    ok = not (R * 4 > 1 << 30 or R * dt >= 65536 or R * D >= 65536)
                    lib.rows_only(lanes, dt, D, batch, 1 << 30, out)
                    assert out[0] == ok and out[1] == R and out[2] == 0 and out[3] == R * 4, (lanes, D, dt, batch)
                    hits.add("ok" if ok else ("R*dt" if R * dt >= 65536 else "R*D only"))
    assert hits == {"ok", "R*dt", "R*D only"}, hits


def test_sample_tiles_of_k2_k4_and_k6(lib):
    out = (ctypes.c_int64 * 12)()
    hits2, hits6 = set(), set()
    for D in D_AXIS:
        for dt in dt_axis(D):
            for batch in batch_axis(first_rows(KB, dt, D, 2 ** 40)):
                for pcols, given in ((dt, 0), (2 * dt, 0), (2 * dt, 1)):   # additive; default / general / softplus; given
                    want = old_k2(D, dt, pcols, given, batch, hits2)
                    lib.k2(D, dt, pcols, given, batch, out)
                    check_tile(out, want, 5, ("K2", D, dt, pcols, given, batch))
                    if want is not None and batch > 0:
                        for cus in CUS:
                            tiles = (batch + want[0] - 1) // want[0]
                            assert lib.grid_lds(cus, want[2], 8, tiles) == old_grid(cus, want[2], 8, tiles)[0]
        for batch in batch_axis(first_rows(4 * KB, 0, D, 2 ** 40)):
            # K4 (nfa_permute_cols_b32): `R = (4 * kBlock) / D`, at least 1, at most the batch
            R = (4 * KB) // D
            if R < 1:
                R = 1
            if R > batch:
                R = batch
            assert lib.k4_rows(D, batch) == R
            for K in K_AXIS:
                for nd in (K - 1, K + 1):
                    want = old_k6(D, K, nd, batch, hits6)
                    lib.k6(D, K, nd, batch, out)
                    check_tile(out, want, 3, ("K6", D, K, nd, batch))
    assert {"halved", "unsupported: tile"} <= hits2, hits2
    assert {"halved", "unsupported: tile"} <= hits6, hits6


def test_element_tiles_of_k5_k9_and_searchsorted(lib):
    """(bin counts beyond the shared axis, up to the ABI's limit of 4096, so that every floor is reached and missed)"""
    hits = {"K5": set(), "K9": set(), "K9 backward": set(), "searchsorted": set()}
    for K in K_AXIS + [64, 300, 1000, 4096]:
        for nd in (K - 1, K + 1):
            P = 2 * K + nd
            for packed in (0, 1):
                want = old_element_tile(1, lambda t: (ru4(t * P) + 8) * 4 if packed else t * (P | 1) * 4, hits["K5"])
                assert lib.k5_tile(P, packed) == want, (K, nd, packed)
        # launch_lq: slot = (K | 2K + 1 | 2K + 2) | 1, floor 32; launch_lq_backward: (K | 5K + 3 | 4K) | 1, floor 64
        for floor, slots, name in ((32, (K, 2 * K + 1, 2 * K + 2), "K9"), (64, (K, 5 * K + 3, 4 * K), "K9 backward")):
            for slot in slots:
                slot |= 1
                want = old_element_tile(floor, lambda t: t * slot * 4, hits[name])
                assert lib.k9_tile(floor, slot) == want, (name, K, slot)
                if want:
                    lds = want * slot * 4 + (64 if floor == 32 else 0)
                    for cus in CUS:
                        for n in (1, want, want + 1, 262144, 2 ** 31 + 5):
                            tiles = (n + want - 1) // want
                            if floor == 32:
                                assert lib.grid_lds(cus, lds, 8, tiles) == old_grid(cus, lds, 8, tiles)[0]
                            else:   # `g = tiles; cap = cus * 8; if (g > cap) g = cap`
                                assert lib.grid_flat(cus, 8, tiles) == min(tiles, cus * 8)
        # nfa_searchsorted_f32's dense rows: K + 1 knots, at most 4096
        if K + 1 <= 4096:
            want = old_element_tile(1, lambda t: (ru4(t * (K + 1)) + 8) * 4, hits["searchsorted"])
            assert lib.search_tile(K + 1) == want
    assert hits["K5"] == {"halved"}, hits        # (one element's logits always fit: 3 * 4096 + 1 floats)
    assert hits["K9"] == {"halved", "unsupported: floor"}, hits
    assert hits["K9 backward"] == {"halved", "unsupported: floor"}, hits
    assert hits["searchsorted"] == {"halved"}, hits


def test_grids_without_an_lds_term(lib):
    """wave_per_row_grid (misc.hip: 8 per CU, at least one), grid_f64 (16 per CU), K4 / searchsorted (8), K7 (2)"""
    for cus in CUS:
        for per_cu in (2, 8, 16):
            for tiles in (0, 1, cus * per_cu - 1, cus * per_cu, cus * per_cu + 1, 65536, 2 ** 31 + 5):
                cap = cus * per_cu
                assert lib.grid_flat(cus, per_cu, tiles) == (cap if tiles > cap else tiles)
