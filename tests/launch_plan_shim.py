"""The host shim of nflows_amd/csrc/launch_plan.hpp: the product's planner compiled for the HOST behind entry points that
lay out LDS the way each launcher's callable does.  tests/test_launch_plan_host.py holds every entry to the launchers'
arithmetic; tests/cdf_shared_cases.py asks `k6` which plan K6 takes at a shape.  CPU only."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include "launch_plan.hpp"
using namespace nfa;
static void put(int64_t* out, const SampleTile& t) { out[0] = t.ok; out[1] = t.R; out[2] = t.C; out[3] = (int64_t)t.lds; }
// K1 forward (nfa_rqs_coupling_f32): out = ok, R, C, lds, off_x, off_out, off_lad, off_idx
extern "C" void k1_forward(int D, int dt, int P, int64_t batch, int64_t* out) {
    auto lds_floats = [&](int r, int chunk) {
        int o = round_up4((chunk > 0 ? chunk : r * dt) * P) + 4;
        out[4] = o;
        o += round_up4(r * D) + 4;
        out[5] = o;
        o += round_up4(r * D) + 4;
        out[6] = o;
        o += round_up4(chunk > 0 ? kBlock : (r * dt > kBlock / kWave ? r * dt : kBlock / kWave));
        out[7] = o;
        o += dt + 2 * D + (D + 3) / 4;
        return o;
    };
    const size_t chunk_fixed = (size_t)(2 * (round_up4(D) + 4) + kBlock + dt + 2 * D + (D + 3) / 4 + 8) * 4;
    put(out, plan_sample_tile(kBlock, dt, D, batch, kDefaultDynLds, lds_floats, P, chunk_fixed));
}
// K1 backward (nfa_rqs_coupling_backward_f32): out = ok, R, C, lds, off_x, off_gy, off_gx, off_idx
extern "C" void k1_backward(int D, int dt, int P, int64_t batch, int64_t* out) {
    auto lds_floats = [&](int r, int chunk) {
        int o = round_up4((chunk > 0 ? chunk : r * dt) * P) + 8;
        out[4] = o;
        o += round_up4(r * D) + 4;
        out[5] = o;
        o += round_up4(r * D) + 4;
        out[6] = o;
        o += round_up4(r * D) + 4;
        out[7] = o;
        o += dt + 2 * D + (D + 3) / 4;
        return o;
    };
    const size_t chunk_fixed = (size_t)(3 * (round_up4(D) + 4) + dt + 2 * D + (D + 3) / 4 + 16) * 4;
    put(out, plan_sample_tile(kBlock, dt, D, batch, kDefaultDynLds, lds_floats, P, chunk_fixed));
}
// K2 (nfa_affine_coupling_f32): out = ok, R, C, lds, off_sc, off_x, off_out, off_lad, off_idx
extern "C" void k2(int D, int dt, int pcols, int given, int64_t batch, int64_t* out) {
    auto lds_floats = [&](int r, int) {
        int o = round_up4(r * pcols) + 4;
        out[4] = o;
        o += (given ? round_up4(r * dt) + 4 : 0);
        out[5] = o;
        o += round_up4(r * D) + 4;
        out[6] = o;
        o += round_up4(r * D) + 4;
        out[7] = o;
        o += round_up4(r * dt);
        out[8] = o;
        o += dt + 2 * D + (D + 3) / 4;
        return o;
    };
    put(out, plan_sample_tile(kBlock, dt, D, batch, kDefaultDynLds, lds_floats));
}
// K6 (nfa_rqs_shared_f32): out = ok, R, C, lds, off_x, off_lad, off_raw
extern "C" void k6(int F, int K, int nd, int64_t batch, int64_t* out) {
    const int64_t tab = (int64_t)F * 3 * (K + 1);
    auto lds_floats = [&](int r, int) {
        int64_t o = (tab + 3) & ~3;
        out[4] = (int)o;
        o += round_up4(r * F) + 8;
        out[5] = (int)o;
        o += round_up4(r * F);
        out[6] = (int)o;
        o += round_up4(F * (2 * K + nd));
        return o;
    };
    put(out, plan_sample_tile(4 * kBlock, 0, F, batch, kDefaultDynLds, lds_floats));
}
// a one-float-per-sample image under a budget of the caller's: the item-count limits decide, not LDS
extern "C" void rows_only(int lanes, int dt, int D, int64_t batch, int64_t budget, int64_t* out) {
    put(out, plan_sample_tile(lanes, dt, D, batch, (size_t)budget, [](int r, int) { return r; }));
}
extern "C" int k4_rows(int D, int64_t batch) { return sample_rows(4 * kBlock, 0, D, batch); }
extern "C" int aligned(int dt, int D, int P, int R, int64_t batch) { return aligned_tile(dt, D, P, R, batch); }
extern "C" int64_t rows_full(int64_t batch, int64_t per_tile) { return full_rows(batch, per_tile); }
// K5 (nfa_rqs_elementwise_f32, floor 1), K9 forward (launch_lq, floor 32) and backward (launch_lq_backward, floor 64),
// searchsorted's dense rows (floor 1): T, or 0
extern "C" int k5_tile(int P, int packed) {
    const int slot = P | 1;
    return plan_element_tile(1, kDefaultDynLds, [&](int t) { return packed ? (size_t)(round_up4(t * P) + 8) * 4 : (size_t)t * slot * 4; });
}
extern "C" int k9_tile(int floor, int slot) {
    return plan_element_tile(floor, kDefaultDynLds, [&](int t) { return (size_t)t * slot * 4; });
}
extern "C" int search_tile(int nk) {
    return plan_element_tile(1, kDefaultDynLds, [&](int t) { return (size_t)(round_up4(t * nk) + 8) * 4; });
}
extern "C" int64_t grid_lds(int cus, int64_t lds, int cap, int64_t tiles) { return persistent_grid(cus, (size_t)lds, cap, tiles); }
extern "C" int64_t grid_flat(int cus, int per_cu, int64_t tiles) { return persistent_grid(cus, per_cu, tiles); }
'''


def build(directory):
    """Compiles the shim into `directory` and returns the library with its argument types set."""
    cpp, so = os.path.join(directory, "launch_plan_host.cpp"), os.path.join(directory, "launch_plan_host.so")
    open(cpp, "w").write(SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "nflows_amd", "csrc"), cpp, "-o", so])
    lib = ctypes.CDLL(so)
    i, l, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    for name, args, res in (("k1_forward", [i, i, i, l, p], None), ("k1_backward", [i, i, i, l, p], None),
                            ("k2", [i, i, i, i, l, p], None), ("k6", [i, i, i, l, p], None),
                            ("rows_only", [i, i, i, l, l, p], None), ("k4_rows", [i, l], i),
                            ("aligned", [i, i, i, i, l], i), ("rows_full", [l, l], l), ("k5_tile", [i, i], i),
                            ("k9_tile", [i, i], i), ("search_tile", [i], i), ("grid_lds", [i, l, i, l], l),
                            ("grid_flat", [i, i, l], l)):
        getattr(lib, name).argtypes = args
        getattr(lib, name).restype = res
    return lib
