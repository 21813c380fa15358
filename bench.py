#!/usr/bin/env python3
"""Headline benchmark: Flow.log_prob throughput of the 32-layer RQ-NSF coupling flow
(dim=64, K=8) on MI355X, with the layer kernel's roofline fraction from the timed steps' own dispatch events.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

The workload is BASELINE configs[3] as named, at every N: a global batch of 262 144 rows, all of them on
the one GPU at N = 1, sharded over the N ranks otherwise (one process per GPU, launched by
torch.distributed.run; 32 768 rows per GPU at N = 8), one 16-byte all-reduce per step.  The total work
is fixed, the per-GPU work shrinks as N grows ("scaling": "strong"); with --full the figure at 65 536 rows per GPU
(round 1's single-GPU workload; weak scaling for N > 1) is added as an extra field.  A "step" is one full log_prob pass over the rank's rows (inputs already
resident in HBM) plus the log-likelihood reduction.  Rank 0 prints ONE JSON line.

A plain run does only what the headline figure needs: set-up, warm-up, the timed steps, --dump-outputs and the result
line.  --full adds everything else after the timed steps: the fwd/inv consistency check and its float64 device path,
the steady-state leg with clock and power, the sustained MFMA ceiling, K1's roofline, the HIP-graph replay, the other
engines, batch sizes and BASELINE configurations, and the reference-CPU-path baseline (oracle/eager.py, the
bit-identical port of the reference's CPU path); the --skip-* options, --no-cpu-baseline and --steady-seconds trim it.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

T_START = time.perf_counter()
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
BF16_PEAK_TFLOPS = 2500.0  # dense bf16 MFMA peak (MI355X_MICROARCH.md; the 5 PFLOP/s headline includes sparsity)


class EventHook:
    """Brackets every K1 launch with HIP events recorded on the stream it is launched on
    (torch's current stream: ops.py passes exactly that handle to the library)."""

    def __init__(self):
        self.pairs = []
        self.bytes = 0
        self.enabled = False

    def begin(self, name):
        if not self.enabled:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, start, nbytes):
        if start is None:
            return
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.pairs.append((start, e))
        self.bytes = nbytes

    def summary(self):
        if not self.pairs:
            return None
        ms = [a.elapsed_time(b) for a, b in self.pairs]
        return sum(ms) / len(ms), len(ms)


def dispatch_durations_ms(capacity):
    """Per-launch K1 durations from the HIP events the library attached to each dispatch
    (hipExtLaunchKernelGGL start/stop events on the launch stream): the kernel's own begin/end
    timestamps, i.e. the quantity rocprofv3's kernel trace reports."""
    import ctypes
    from nflows_amd import _native
    buf = (ctypes.c_float * capacity)()
    n = ctypes.c_int32(0)
    _native.check(_native.load().nfa_profile_collect(buf, capacity, ctypes.byref(n)))
    return [buf[i] for i in range(n.value)]


class SmiSampler:
    """Shader clock and socket power from `rocm-smi`, sampled from a thread while a measurement leg runs (the
    headline kernel is limited by the chip's power cap, DESIGN.md section 4: the clock it sustains is part of
    the measurement)."""

    def __init__(self):
        self.samples = []
        self._stop = False
        self._thread = None

    @staticmethod
    def read():
        import re
        import subprocess
        try:
            out = subprocess.run(["rocm-smi", "--showclocks", "--showpower"], capture_output=True, text=True, timeout=10).stdout
        except Exception:
            return None
        c = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", out)
        p_ = re.search(r"Graphics Package Power \(W\): ([\d.]+)", out)
        return (int(c.group(1)) if c else None, float(p_.group(1)) if p_ else None)

    def _run(self):
        while not self._stop:
            r = self.read()
            if r is not None:
                self.samples.append(r)
            time.sleep(0.25)

    def __enter__(self):
        import threading
        self._thread = threading.Thread(target=self._run, daemon=True)
        self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop = True
        self._thread.join(timeout=15)

    def summary(self):
        import statistics
        clk = [c for c, _ in self.samples if c]
        pw = [p_ for _, p_ in self.samples if p_]
        if not clk and not pw:
            return None
        return {"sclk_mhz_median": statistics.median(clk) if clk else None, "sclk_mhz_min": min(clk) if clk else None,
                "socket_power_w_median": statistics.median(pw) if pw else None, "samples": len(self.samples),
                "source": "rocm-smi --showclocks --showpower, sampled during the steady-state leg"}


def sustained_mfma_ceiling(seconds=1.5):
    """tools/bin/mfma_power_probe (built by __graft_entry__.build): the f16 matrix pipe's back-to-back rate
    under the power cap with zero and with Gaussian operands, measured on this box.  None if the probe is absent."""
    import re
    import subprocess
    exe = os.path.join(ROOT, "tools", "bin", "mfma_power_probe")
    if not os.path.exists(exe):
        return None
    try:
        out = subprocess.run([exe, str(seconds)], capture_output=True, text=True, timeout=120).stdout
    except Exception:
        return None
    res = {}
    for kind, shape, val in re.findall(r"mfma_power_probe (\w+) (\w+): ([\d.]+) TFLOP/s", out):
        res["%s_%s" % (kind, shape)] = float(val)
    return res or None


# the sources that define each profiled kernel: a counter file under profiles/ is only quoted while they are unchanged
KERNEL_SOURCES = {
    "k8h_pmc_traffic.json": ("rqs_resnet_f16_kernel.hpp", "rqs_resnet_f16.hip", "k8h_common.hpp", "rqs_fused8.hpp", "rqs_math.hpp",
                             "fused_common.hpp", "common.hpp"),
    "k8_pmc_traffic.json": ("rqs_resnet_kernel.hpp", "rqs_resnet.hip", "bf16x3_gemm.hpp", "rqs_math.hpp", "fused_common.hpp",
                            "common.hpp"),
    "k8x_pmc_traffic.json": ("rqs_resnet_f16x3.hip", "rqs_resnet_f16x3_kernel.hpp", "f16x3_gemm.hpp", "bf16x3_gemm.hpp", "rqs_resnet_f16_kernel.hpp", "k8h_common.hpp",
                             "rqs_fused8.hpp", "rqs_math.hpp", "fused_common.hpp", "common.hpp"),
    "k7b_pmc_traffic.json": ("rqs_fused_linear.hip", "rqs_math.hpp", "fused_common.hpp", "common.hpp"),
    "k7_pmc_traffic.json": ("rqs_fused_linear.hip", "rqs_math.hpp", "fused_common.hpp", "common.hpp"),
    "k1_pmc_traffic.json": ("rqs.hip", "rqs_math.hpp", "common.hpp"),
}


def kernel_source_digest(traffic_file):
    """sha256 over the kernel's source files (tools/pmc_traffic.py stores it next to the counters it collects)."""
    import hashlib
    h = hashlib.sha256()
    for name in KERNEL_SOURCES[traffic_file]:
        with open(os.path.join(ROOT, "nflows_amd", "csrc", name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()


def log(msg):
    print("[bench %.1fs] %s" % (time.perf_counter() - T_START, msg), file=sys.stderr, flush=True)


def usable_cores():
    """Host cores this process may actually use: affinity mask, capped by the cgroup CPU quota."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period))))
    except Exception:
        pass
    return n


def dump_outputs(out_dir, log_prob, acc, rank, world, limit_bytes=64 << 20):
    """--dump-outputs: what the timed step handed its caller in the LAST timed step -- the per-row log-densities of this
    rank's rows (log_prob.npy, float32) and the (sum, count) the log-likelihood reduction returned (log_likelihood_sum_count.npy,
    float64) -- so that two builds can be compared output for output on the same seeded inputs.  At most `limit_bytes` in
    all: log-densities beyond that are cut to a fixed, seeded sample of rows, whose indices go to log_prob_rows.npy
    (float64).  Ranks other than 0 add _rank<r> to the names and share the limit."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    suffix = "" if world == 1 else "_rank%d" % rank
    lp = log_prob.detach().float().cpu().numpy().reshape(-1)
    budget = limit_bytes // world - 4096
    written = {}
    if lp.nbytes > budget:
        n = budget // (4 + 8)
        rows = np.sort(np.random.RandomState(0).choice(lp.size, n, replace=False))
        lp = lp[rows]
        written["log_prob_rows"] = rows.astype(np.float64)
    written["log_prob"] = np.ascontiguousarray(lp, dtype=np.float32)
    written["log_likelihood_sum_count"] = acc.detach().double().cpu().numpy().reshape(-1)
    for name, arr in written.items():
        np.save(os.path.join(out_dir, name + suffix + ".npy"), arr)
    log("outputs of the last timed step written to %s: %s" % (out_dir, ", ".join(
        "%s%s.npy %s" % (k, suffix, list(v.shape)) for k, v in written.items())))


def cpu_baseline(flow_cpu, features, sample_rows, x_consistency=None, budget_s=20.0, full_rows=0):
    """The reference's CPU path on the host cores this process may use: its bit-identical PyTorch-eager
    port (oracle/eager.py; tests/test_oracle_golden.py pins it bit for bit).  Bounded:
    rows are reduced until one pass fits the time budget.  Also reports a one-thread figure and the
    reference's own forward/inverse consistency error on the rows bench.py uses for the HIP path."""
    from oracle import eager
    threads = usable_cores()
    kind = "port"

    def run(x):
        return eager.flow_log_prob(flow_cpu, x)

    def timed(rows, nthreads, budget):
        torch.set_num_threads(nthreads)
        while True:
            x = torch.randn(rows, features, generator=torch.Generator().manual_seed(1234))
            t0 = time.perf_counter()
            run(x)  # warm-up pass, also the probe
            probe = time.perf_counter() - t0
            log("cpu baseline (%s, %d threads): %d rows, probe pass %.2f s" % (kind, nthreads, rows, probe))
            if probe <= budget / 4 or rows <= 512:
                break
            rows //= 4
        reps = max(1, min(3, int(budget / max(probe, 1e-3)) - 1))
        t0 = time.perf_counter()
        for _ in range(reps):
            run(x)
        return rows, reps, (time.perf_counter() - t0) / reps

    with torch.no_grad():
        rows, reps, dt = timed(sample_rows, threads, budget_s * 0.6)
        rows1, reps1, dt1 = timed(max(512, sample_rows // 8), 1, budget_s * 0.25)
        consistency = None
        if x_consistency is not None:
            torch.set_num_threads(threads)
            xs = x_consistency
            z, _ = eager.flow_transform(flow_cpu, xs)
            xr, _ = eager.flow_transform(flow_cpu, z, inverse=True)
            err = (xr - xs).abs()
            consistency = {"max": err.max().item(), "mean": err.mean().item(),
                           "q999": torch.quantile(err.flatten()[:2 ** 24].double(), 0.999).item(),
                           "count_above_1e-3": int((err > 1e-3).sum().item()), "rows": xs.shape[0]}
    full = None
    if full_rows and full_rows > rows:
        # BASELINE's own batch (65 536 rows), ONE pass (the reference is ~2 x slower per sample there than at the sample size:
        # its [N, 8] intermediates leave the caches)
        with torch.no_grad():
            torch.set_num_threads(threads)
            xf = torch.randn(full_rows, features, generator=torch.Generator().manual_seed(1234))
            t0 = time.perf_counter()
            run(xf)
            dtf = time.perf_counter() - t0
        full = {"rows": full_rows, "passes": 1, "seconds": dtf, "value": full_rows / dtf, "unit": "samples/s", "cores": threads}
        log("cpu baseline at %d rows: one pass %.1f s" % (full_rows, dtf))
    out = {"value": rows / dt, "unit": "samples/s", "cores": threads, "kind": kind,
           "sample": "same 32-layer flow and weights, %d rows x %d timed passes of %s, %.2f s/pass"
                     % (rows, reps, "oracle/eager.py (bit-identical port of the reference CPU path)", dt),
           "one_thread": {"value": rows1 / dt1, "unit": "samples/s", "rows": rows1, "passes": reps1}}
    if full is not None:
        out["at_baseline_batch"] = full
    if consistency is not None:
        out["reference_fwd_inv_err_same_rows"] = consistency
    return out


def other_configs(dev, steps):
    """The other BASELINE.json configurations on this GPU, outside the timed region (`other_configs_extra`): configs[1]
    (8 affine couplings, D = 32, MLP conditioner, 16 384 rows: K11, one launch), configs[2] (16 RQ couplings, D = 64, K = 8,
    65 536 rows: the headline's kernel), configs[4] (autoregressive RQ spline, D = 784, K = 8, 4 096 rows: forward K13, full
    inverse K12 + K13).  Per entry: ms per pass, samples/s, the layer kernel the library launched last, and that pass in
    the unit of its bound -- HBM GB/s over SURVEY 8d's algorithmic bytes and / or the fp32 multiply-adds of its GEMMs."""
    from nflows_amd import configs, ops
    from nflows_amd.transforms import PiecewiseRationalQuadraticCouplingTransform as RQ
    out = []

    def timed(fn, reps, warm):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    def entry(name, seconds, rows, bytes_per_row=None, macs_per_row=None, **extra):
        e = dict(config=name, ms=seconds * 1e3, samples_per_s=rows / seconds, rows=rows, kernel=ops.last_layer_kernel(), **extra)
        if bytes_per_row is not None:
            e["hbm"] = {"algorithmic_bytes": rows * bytes_per_row, "achieved_gbs": rows * bytes_per_row / seconds / 1e9,
                        "frac_of_8000": rows * bytes_per_row / seconds / 1e9 / HBM_PEAK_GBS}
        if macs_per_row is not None:
            tf = 2.0 * rows * macs_per_row / seconds / 1e12
            e["gemm"] = {"fp32_flops": 2.0 * rows * macs_per_row, "achieved_tflops": tf, "frac_of_16bit_mfma_peak": tf / BF16_PEAK_TFLOPS,
                         "frac_of_fp32_matrix_peak": tf / 157.3}
        out.append(e)

    with torch.no_grad():
        try:   # configs[1]
            flow = configs.affine_coupling_flow(8, 32, (128, 128)).to(dev).eval()
            x = torch.randn(16384, 32, device=dev)
            macs = 8 * (16 * 128 + 128 * 128 + 128 * 32)
            entry("configs[1] 8 x AffineCouplingTransform, D=32, MLP 128x128, log_prob", timed(lambda: flow.log_prob(x), 100, 100), 16384,
                  bytes_per_row=4 * (32 + 1), macs_per_row=macs)
            z, _ = flow._transform(x)
            xr, _ = flow._transform.inverse(z)
            entry("configs[1] inverse (sampling direction)", timed(lambda: flow._transform.inverse(z), 100, 100), 16384,
                  bytes_per_row=4 * (32 + 32 + 1), macs_per_row=macs, fwd_inv_max_err=(xr - x).abs().max().item())
            del flow
        except Exception as e:
            log("other_configs: configs[1] skipped: %r" % (e,))
        try:   # configs[2]
            flow = configs.rq_nsf_flow(16, 64, 8, 128).to(dev).eval()
            x = torch.randn(65536, 64, device=dev)
            macs = 16 * (32 * 23 * 128 + 32 * 128 + 4 * 128 * 128)
            for engine in ("f16x3", "f16x2"):
                saved = RQ.conditioner_engine
                try:
                    RQ.conditioner_engine = engine
                    entry("configs[2] 16 x RQ coupling, D=64, K=8, ResidualNet, log_prob, engine %s" % engine,
                          timed(lambda: flow.log_prob(x), max(10, steps), 5), 65536, bytes_per_row=16 * 3460, macs_per_row=macs, engine=engine)
                    if engine == "f16x3":
                        z, _ = flow._transform(x)
                        xr, _ = flow._transform.inverse(z)
                        entry("configs[2] inverse (sampling direction), engine f16x3", timed(lambda: flow._transform.inverse(z), max(10, steps), 5),
                              65536, bytes_per_row=16 * 3460, macs_per_row=macs, engine=engine, fwd_inv_max_err=(xr - x).abs().max().item())
                finally:
                    RQ.conditioner_engine = saved
            del flow
        except Exception as e:
            log("other_configs: configs[2] skipped: %r" % (e,))
        try:   # configs[4]
            flow = configs.ar_rq_flow(784, 256, 8, 3.0, 2).to(dev).eval()
            x = torch.randn(4096, 784, device=dev)
            t = flow._transform._transforms[0]
            macs = 784 * 256 + 4 * 256 * 256 + 256 * 784 * 23      # MADE: initial, two blocks, output layer
            entry("configs[4] MaskedPiecewiseRationalQuadraticAutoregressive, D=784, K=8, log_prob (forward)",
                  timed(lambda: flow.log_prob(x), 20, 5), 4096, bytes_per_row=78404, macs_per_row=macs)
            z = torch.randn(4096, 784, device=dev)
            xs, _ = t.inverse(z)
            zz, _ = t(xs)
            entry("configs[4] FULL inverse (the sampling path: 784 sequential features)", timed(lambda: t.inverse(z), 10, 3), 4096,
                  fwd_of_inverse_max_err=(zz - z).abs().max().item(),
                  note="sequential part in one persistent kernel (K12), the rest K13; the reference runs 784 full passes")
            del flow
        except Exception as e:
            log("other_configs: configs[4] skipped: %r" % (e,))
        try:   # the reference constructor's DEFAULT coupling (num_bins=10, tails=None: coupling.py:503-515), not a BASELINE config
            from nflows_amd.transforms import CompositeTransform, RandomPermutation
            from nflows_amd.nn.nets import ResidualNet
            from nflows_amd.utils import torchutils
            torch.manual_seed(0)
            t = CompositeTransform(sum([[RandomPermutation(64), RQ(torchutils.create_alternating_binary_mask(64, even=(i % 2 == 0)),
                                         lambda a, b: ResidualNet(a, b, hidden_features=128, num_blocks=2), num_bins=10, tails=None)]
                                        for i in range(32)], [])).to(dev).eval()
            x = torch.rand(65536, 64, device=dev) * 0.98 + 0.01
            macs = 32 * (32 * 31 * 128 + 32 * 128 + 4 * 128 * 128)
            entry("default constructor: 32 x RQ coupling, D=64, num_bins=10, tails=None (constrained spline on [0, 1]), forward",
                  timed(lambda: t(x), max(10, steps), 3), 65536, bytes_per_row=32 * (256 + 32 * 31 * 4 + 256 + 4), macs_per_row=macs)
            saved = (RQ.fuse_conditioner, RQ.fuse_final_linear)
            try:
                RQ.fuse_conditioner = RQ.fuse_final_linear = False
                entry("the same, layer by layer (library GEMMs + K1)", timed(lambda: t(x), 5, 2), 65536,
                      bytes_per_row=32 * (256 + 32 * 31 * 4 + 256 + 4), macs_per_row=macs)
            finally:
                RQ.fuse_conditioner, RQ.fuse_final_linear = saved
            del t
        except Exception as e:
            log("other_configs: tails=None flow skipped: %r" % (e,))
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch-per-gpu", type=int, default=None,
                    help="rows per GPU (default: 262144 / N: BASELINE configs[3] over the N GPUs)")
    ap.add_argument("--steady-seconds", type=float, default=1.0,
                    help="length of the additional steady-state measurement (extra field; 0 = skip)")
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-rows", type=int, default=16384)
    ap.add_argument("--no-fuse", action="store_true", help="run permutations as separate kernels")
    ap.add_argument("--path", choices=["k8", "k7b", "k7", "k1"], default="k8",
                    help="layer kernel: k8 = whole ResidualNet conditioner + spline in one kernel "
                         "(default), k7b / k7 = only the final Linear fused (split-bf16 / fp32 MFMA), "
                         "k1 = PyTorch conditioner + spline kernel")
    ap.add_argument("--engine", choices=["f16x3", "f16x2", "bf16x3"], default="f16x3",
                    help="GEMM engine of the whole-layer kernel (--path k8): f16x3 = K8x, three f16 pieces per operand, five "
                         "products: operands at the reference's fp32 width (default, the headline); f16x2 = K8h / K8s, two f16 "
                         "pieces, three products (22-bit operand significands; timed as an extra); bf16x3 = K8, three bf16 pieces")
    ap.add_argument("--no-fuse-linear", action="store_true",
                    help="leave the conditioner's final Linear to hipBLASLt (GEMM + K1 instead of K7)")
    ap.add_argument("--skip-k1-roofline", action="store_true")
    ap.add_argument("--skip-mfma-ceiling", action="store_true",
                    help="do not run tools/bin/mfma_power_probe (the sustained MFMA ceiling under the power cap, ~6 s)")
    ap.add_argument("--skip-graph", action="store_true",
                    help="do not add the HIP-graph replay timing of the same step (extra field)")
    ap.add_argument("--bracket-events", action="store_true",
                    help="additionally bracket every K1 launch with torch events (includes launch gaps)")
    ap.add_argument("--skip-extra", action="store_true",
                    help="skip the extra measurement at 65 536 rows per GPU (profiling runs: one launch size in the trace)")
    ap.add_argument("--skip-consistency", action="store_true",
                    help="skip the fwd/inv check (profiling runs: only full-batch launches in the trace)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (per-row log-densities, log-likelihood sum and count) "
                         "as DIR/<name>.npy, at most 64 MB in all")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline figure, after the timed steps (see the "
                         "module docstring); without it a run does set-up, warm-up, the timed steps, --dump-outputs and "
                         "the result line only")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if not args.full:
        args.steady_seconds = 0
        args.no_cpu_baseline = args.skip_extra = args.skip_consistency = True
        args.skip_mfma_ceiling = args.skip_k1_roofline = args.skip_graph = True

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the measured path)")
    # NFA_BENCH_BACKEND=gloo: dry run of the multi-rank control flow on a box with fewer GPUs than
    # ranks (ranks share devices; numbers are meaningless) -- the real runs use RCCL
    backend = os.environ.get("NFA_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    if args.gpus != world and rank == 0:
        print("note: --gpus %d but WORLD_SIZE=%d; using WORLD_SIZE" % (args.gpus, world), file=sys.stderr)

    import nflows_amd
    from nflows_amd import configs, ops, parallel
    log("imports done; building flow")

    D, K, H = 64, 8, 128
    flow_cpu = configs.rq_nsf_flow(num_layers=args.layers, features=D, num_bins=K, hidden_features=H,
                                   num_blocks=2, tail_bound=3.0, seed=0).eval()  # same seed on every rank
    import copy
    flow = copy.deepcopy(flow_cpu).to(dev)
    flow._transform.fuse_permutations = not args.no_fuse
    from nflows_amd.transforms import PiecewiseRationalQuadraticCouplingTransform as RQ

    def select_path(path):
        RQ.fuse_conditioner = path == "k8"
        RQ.fuse_final_linear = path != "k1"
        RQ.final_linear_engine = "f32" if path == "k7" else "bf16x3"

    if args.no_fuse_linear:
        args.path = "k1"
    select_path(args.path)
    RQ.conditioner_engine = args.engine
    CONFIG4_GLOBAL = 262144
    if args.batch_per_gpu is not None:
        B = args.batch_per_gpu
    else:
        lo, hi = parallel.row_block(CONFIG4_GLOBAL, rank, world)
        B = hi - lo
    x = torch.randn(B, D, generator=torch.Generator().manual_seed(1234 + rank)).to(dev)

    log("flow on device; warm-up")
    hook = EventHook()
    ops.set_launch_hook(hook)

    def step():
        with torch.no_grad():
            lp = flow.log_prob(x)
        return lp, parallel.reduce_log_likelihood(lp)

    for _ in range(args.warmup):
        lp, acc = step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    log("warm-up done; timing %d steps" % args.steps)
    hook.enabled = args.bracket_events
    from nflows_amd import _native
    max_launches = args.layers * args.steps
    _native.check(_native.load().nfa_profile_enable(max_launches))
    t0 = time.perf_counter()
    for _ in range(args.steps):
        lp, acc = step()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    hook.enabled = False
    k1_ms = dispatch_durations_ms(max_launches)
    _native.check(_native.load().nfa_profile_enable(0))
    log("timed region done: %.1f ms/step" % (elapsed / args.steps * 1e3))
    nflows_amd.check_status()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, lp, acc, rank, world)
    del lp
    # 128-row blocks of the last timed step that left the f16 range and were redone by the exact kernel
    # (K8h only; 0 = the whole batch ran on the measured kernel)
    redo_blocks = ops.last_redo_blocks() if args.path == "k8" else None
    # the instance the library launched last in the timed region (the launchers choose it from the rank's batch, the
    # CU count and the LDS budget: at N = 8 a rank's 32 768 rows run K8s, not K8h)
    timed_kernel = ops.last_layer_kernel()

    t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = t.item()
    mean_ll = (acc[0] / acc[1]).item()

    # steady state: the same step repeated for >= --steady-seconds (the timed region above is
    # K steps of a few milliseconds; this one shows what a long-running job sustains)
    steady = None
    if args.steady_seconds > 0:
        n_batch = max(10, args.steps)
        done, t0 = 0, time.perf_counter()
        if world > 1:
            dist.barrier()
        smi = SmiSampler() if rank == 0 else None
        if smi is not None:
            smi.__enter__()
        while True:
            for _ in range(n_batch):
                step()
            torch.cuda.synchronize()
            done += n_batch
            stop = torch.tensor([1.0 if time.perf_counter() - t0 >= args.steady_seconds else 0.0], device=dev)
            if world > 1:
                dist.all_reduce(stop, op=dist.ReduceOp.MAX)
            if stop.item() > 0:
                break
        if world > 1:
            dist.barrier()
        dt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(dt, op=dist.ReduceOp.MAX)
        steady = {"steps": done, "seconds": dt.item(), "ms_per_step": dt.item() / done * 1e3}
        if smi is not None:
            smi.__exit__()
            steady["clock_and_power"] = smi.summary()
    # extra: 65 536 rows on every GPU (round 1's single-GPU workload; weak scaling for N > 1)
    weak = None
    if args.batch_per_gpu is None and not args.skip_extra:
        xw = torch.randn(65536, D, generator=torch.Generator().manual_seed(4321 + rank)).to(dev)

        def step_w():
            with torch.no_grad():
                return parallel.reduce_log_likelihood(flow.log_prob(xw))
        for _ in range(3):
            step_w()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        tw = time.perf_counter()
        for _ in range(args.steps):
            step_w()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()
        dtw = torch.tensor([time.perf_counter() - tw], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(dtw, op=dist.ReduceOp.MAX)
        weak = {"rows_per_gpu": 65536, "ms_per_step": dtw.item() / args.steps * 1e3,
                "value": 65536 * world * args.steps / dtw.item(), "unit": "samples/s"}
        del xw

    # extra (N = 1): the shards config 4 leaves a GPU at 8 / 16 / 32 GPUs -- the small-batch kernels (K8s: 128-row
    # blocks at 32 768 rows; K8c, round 6: column-split 64-row blocks below), same step as the headline
    small = None
    if world == 1 and args.batch_per_gpu is None and not args.skip_extra:
        small = []
        for rows_s in (32768, 16384, 8192):
            xs_ = torch.randn(rows_s, D, generator=torch.Generator().manual_seed(977 + rows_s)).to(dev)

            def step_s():
                with torch.no_grad():
                    return parallel.reduce_log_likelihood(flow.log_prob(xs_))
            for _ in range(5):
                step_s()
            torch.cuda.synchronize()
            ts = time.perf_counter()
            for _ in range(args.steps):
                step_s()
            torch.cuda.synchronize()
            dts = time.perf_counter() - ts
            entry_s = {"rows": rows_s, "ms_per_step": dts / args.steps * 1e3, "value": rows_s * args.steps / dts,
                       "unit": "samples/s", "engine": args.engine, "kernel": ops.last_layer_kernel()}
            if args.engine != "f16x2" and args.path == "k8":
                # (the library's small-batch kernels -- K8s, 16-sample tiles -- exist for the two-piece engine only)
                try:
                    RQ.conditioner_engine = "f16x2"
                    for _ in range(5):
                        step_s()
                    torch.cuda.synchronize()
                    ts = time.perf_counter()
                    for _ in range(args.steps):
                        step_s()
                    torch.cuda.synchronize()
                    dt2 = time.perf_counter() - ts
                    entry_s["engine_f16x2"] = {"ms_per_step": dt2 / args.steps * 1e3, "value": rows_s * args.steps / dt2,
                                               "kernel": ops.last_layer_kernel()}
                    if ops.use_tile16(rows_s, K, None, dev) == 2:   # K8c's batches: K8s (the kernel of rounds 3-5) beside it
                        saved_c = ops.K8C_ENABLED
                        try:
                            ops.K8C_ENABLED = False
                            for _ in range(5):
                                step_s()
                            torch.cuda.synchronize()
                            ts = time.perf_counter()
                            for _ in range(args.steps):
                                step_s()
                            torch.cuda.synchronize()
                            dt3 = time.perf_counter() - ts
                            entry_s["engine_f16x2_k8s"] = {"ms_per_step": dt3 / args.steps * 1e3, "value": rows_s * args.steps / dt3,
                                                           "kernel": ops.last_layer_kernel()}
                        finally:
                            ops.K8C_ENABLED = saved_c
                finally:
                    RQ.conditioner_engine = args.engine
            small.append(entry_s)
            del xs_

    # extra (N = 1): the same step on every OTHER engine -- K8h (two f16 pieces, three products: the fastest, 22-bit operand
    # significands), K8 (three bf16 pieces, six products), and layer by layer (PyTorch / hipBLASLt fp32 conditioner + K1) --,
    # each timed like the headline (the same number of steps, per-dispatch HIP events for its roofline block)
    other_engines = None
    if world == 1 and args.batch_per_gpu is None and not args.skip_extra and args.path == "k8":
        other_engines = []
        candidates = [("K8x: whole-layer kernel on three f16 pieces per operand (5 products: operands at fp32 width)", "f16x3", "k8"),
                      ("K8h: whole-layer kernel on two f16 pieces per operand (3 products, 22-bit operand significands)", "f16x2", "k8"),
                      ("K8: whole-layer kernel on three bf16 pieces per operand (6 products, 24-bit significands)", "bf16x3", "k8"),
                      ("layer by layer: PyTorch (hipBLASLt) fp32 conditioner GEMMs + K1 spline kernel", args.engine, "k1")]
        for label, engine, path in candidates:
            if path == "k8" and engine == args.engine:
                continue
            try:
                RQ.conditioner_engine = engine
                select_path(path)
                flow_e = copy.deepcopy(flow_cpu).to(dev)
                flow_e._transform.fuse_permutations = not args.no_fuse

                def step_e():
                    with torch.no_grad():
                        return parallel.reduce_log_likelihood(flow_e.log_prob(x))
                for _ in range(3):
                    acc_e = step_e()
                torch.cuda.synchronize()
                n_e = max(20, args.steps) if path == "k8" else max(10, args.steps // 2)
                _native.check(_native.load().nfa_profile_enable(args.layers * n_e))
                te = time.perf_counter()
                for _ in range(n_e):
                    acc_e = step_e()
                torch.cuda.synchronize()
                dte = (time.perf_counter() - te) / n_e
                ms_e = dispatch_durations_ms(args.layers * n_e)
                _native.check(_native.load().nfa_profile_enable(0))
                other_engines.append({"engine": label, "kernel": ops.last_layer_kernel(), "rows": B, "steps": n_e,
                                      "ms_per_step": dte * 1e3, "value": B / dte, "unit": "samples/s",
                                      "mean_log_likelihood": (acc_e[0] / acc_e[1]).item(),
                                      "redo_blocks": ops.last_redo_blocks() if (path == "k8" and engine != "bf16x3") else None,
                                      "_roofline_args": (path, engine, ms_e, len(ms_e) / n_e)})
                del flow_e
            except Exception as e:  # measurement extra only
                log("engine extra (%s / %s) skipped: %r" % (path, engine, e))
            finally:
                _native.load().nfa_profile_enable(0)
                RQ.conditioner_engine = args.engine
                select_path(args.path)
        torch.cuda.empty_cache()

    # the same step replayed from a HIP graph (host out of the loop): reported beside the headline
    # number, which keeps per-dispatch events and therefore launches from the host
    graph_ms = None
    if world == 1 and not args.skip_graph:
        try:
            from nflows_amd.graphs import GraphedLogProb
            g = GraphedLogProb(flow, x)
            for _ in range(3):
                parallel.reduce_log_likelihood(g(x))
            torch.cuda.synchronize()
            tg = time.perf_counter()
            for _ in range(args.steps):
                acc_g = parallel.reduce_log_likelihood(g(x))
            torch.cuda.synchronize()
            graph_ms = (time.perf_counter() - tg) / args.steps * 1e3
            assert abs((acc_g[0] / acc_g[1]).item() - mean_ll) < 1e-6 * abs(mean_ll)
            del g
        except Exception as e:  # measurement extra only
            log("HIP-graph timing skipped: %r" % (e,))

    # forward∘inverse consistency (second half of the metric), outside the timed region
    err_composite = err_layer = err_stats = None
    xs = x[:8192]
    with torch.no_grad():
        if not args.skip_consistency:
            z, lad = flow._transform(xs)
            xr, lad_inv = flow._transform.inverse(z)
            err_t = (xr - xs).abs()
            err_composite = err_t.max().item()
            err_stats = {"mean": err_t.mean().item(), "q999": torch.quantile(err_t.flatten().double(), 0.999).item(),
                         "count_above_1e-3": int((err_t > 1e-3).sum().item())}
            layer = flow._transform._transforms[1]
            y1, _ = layer(xs)
            x1, _ = layer.inverse(y1)
            err_layer = (x1 - xs).abs().max().item()
    # the second half of the metric asks for < 1e-5: neither the reference nor anything else meets that in fp32 on 32
    # layers.  The same rows through the float64 device path (`flow.double()`: K5d spline kernel, library
    # fp64 GEMMs) -- the configuration in which the target IS met, by the reference and here
    fp64_extra = None
    if world == 1 and not args.skip_consistency and not args.skip_extra:
        try:
            flow64 = copy.deepcopy(flow_cpu).double().to(dev)
            x64 = xs.double()
            with torch.no_grad():
                z64, _ = flow64._transform(x64)
                xr64, _ = flow64._transform.inverse(z64)
                e64 = (xr64 - x64).abs()
                lp64 = flow64.log_prob(x64)
                torch.cuda.synchronize()
                t64 = time.perf_counter()
                for _ in range(3):
                    flow64.log_prob(x64)
                torch.cuda.synchronize()
                dt64 = (time.perf_counter() - t64) / 3
                lp32 = flow.log_prob(xs)
            graph64 = None
            try:   # the same pass replayed from a HIP graph: ~25 small launches per layer, the host out of the loop
                from nflows_amd.graphs import GraphedLogProb
                g64 = GraphedLogProb(flow64, x64)
                for _ in range(2):
                    g64(x64)
                torch.cuda.synchronize()
                tg64 = time.perf_counter()
                for _ in range(5):
                    out64 = g64(x64)
                torch.cuda.synchronize()
                dtg = (time.perf_counter() - tg64) / 5
                graph64 = {"log_prob_ms": dtg * 1e3, "log_prob_samples_per_s": x64.shape[0] / dtg,
                           "bit_identical_to_eager_launches": bool(torch.equal(out64, lp64))}
                del g64
            except Exception as e:
                log("fp64 graph replay skipped: %r" % (e,))
            fp64_extra = {"rows": int(x64.shape[0]), "dtype": "f64", "max": e64.max().item(), "mean": e64.mean().item(),
                          "count_above_1e-5": int((e64 > 1e-5).sum().item()), "meets_1e-5": bool(e64.max().item() < 1e-5),
                          "log_prob_ms": dt64 * 1e3, "log_prob_samples_per_s": x64.shape[0] / dt64,
                          "max_abs_log_prob_f32_minus_f64": (lp32.double() - lp64).abs().max().item(),
                          "hip_graph_replay": graph64,
                          "note": "flow.double() on the device: float64 spline kernel (nfa_rqs_elementwise_f64) + library fp64 GEMMs, "
                                  "layer by layer; not a fast path"}
            del flow64
        except Exception as e:  # measurement extra only
            log("fp64 extra skipped: %r" % (e,))

    if rank == 0:
        total_rows = (CONFIG4_GLOBAL if (world > 1 and args.batch_per_gpu is None) else B * world)
        H_ = 128
        P_ = 3 * K - 1
        dt_ = D // 2
        nb_ = 2
        k1_bytes = 4 * (B * D + B * dt_ * P_ + B * D + B)  # 3460 B/sample/layer
        io_bytes = 4 * (B * D + B * D + B)                 # inputs + outputs + logabsdet

        def load_traffic(name):
            """(bytes per launch, provenance): the counters of profiles/<name> -- refused (None) when the kernel's
            sources have changed since tools/pmc_traffic.py collected them (the file records their digest)."""
            try:
                rec = json.load(open(os.path.join(ROOT, "profiles", name)))
            except Exception:
                return None, "profiles/%s: absent" % name
            want = rec.get("kernel_source_sha256")
            have = kernel_source_digest(name) if name in KERNEL_SOURCES else None
            if want is None or want != have:
                return None, ("profiles/%s was collected on other kernel sources (digest %s, now %s): not quoted; "
                              "re-run tools/collect_profiles.sh" % (name, str(want)[:12], str(have)[:12]))
            return rec.get("hbm_bytes_per_launch"), ("profiles/%s (rocprofv3 --pmc passes of this command on these kernel "
                                                     "sources, digest %s; not re-measured in this run)" % (name, have[:12]))

        timing_note = ("HIP start/stop events attached to each layer-kernel dispatch on its launch "
                       "stream (hipExtLaunchKernelGGL), all launches of the timed region")

        # pieces per operand, products per multiply-add, the same in instruction TIME at the 16-bit rate (K8x: its two
        # 2^-22-level products run on the bf8 MX instruction, twice the f16 rate: 3 + 2 / 2), pipe, weight-stream bytes per
        # layer, counter file
        ENGINES = {
            "f16x3": ("three f16 pieces (33 significand bits: the fp32 operand exactly; the two smallest of the five cross "
                      "products from the pieces' high bytes on v_mfma_scale_f32_32x32x64_f8f6f4, bf8 x bf8)", 5, 4.0, "f16 + bf8",
                      (2 + 16 * nb_ + 2 * (dt_ * 24 // 32)) * 12288, "k8x_pmc_traffic.json"),
            "f16x2": ("two f16 pieces (22 significand bits)", 3, 3.0, "f16",
                      (2 + 8 * nb_ + dt_ * 24 // 32) * 16384, "k8h_pmc_traffic.json"),   # (+ the parameter stage)
            "bf16x3": ("three bf16 pieces (24 significand bits)", 6, 6.0, "bf16",
                       (2 + 16 * nb_ + 2 * (dt_ * 24 // 32)) * 12288, "k8_pmc_traffic.json"),
        }

        def roofline_of(path, ms, launches_per_step, ran=None, engine=None):
            """`launches_per_step` layer-kernel dispatches make one step of `args.layers` layers: 32
            (one layer per launch) or 1 (the run of K8 layers in a single launch).  `ran`: the kernel name the
            library reported (nfa_last_layer_kernel) -- `kernel` is then that name, not a guess."""
            engine = engine or args.engine
            avg_ms, launches = sum(ms) / len(ms), len(ms)
            layers_per_launch = args.layers / launches_per_step
            common = {"avg_launch_ms": avg_ms, "launches_timed": launches, "layers_per_launch": layers_per_launch,
                      "timing": timing_note}
            if path in ("k8", "k7b"):
                # `achieved` follows SURVEY 8d: the fp32 multiply-adds of the layers' GEMMs (x 2 flop), unpadded -- the work the
                # reference's F.linear calls do -- over the launch duration.  The kernels do that work on the 16-bit matrix
                # pipe with split operands: `matrix_pipe` says what the pipe itself executed
                # (products per multiply-add x the same flops) and how busy that kept it.
                pieces, products, slots, pipe, weight_bytes, traffic_file = ENGINES[engine] if path == "k8" else \
                    ("three bf16 pieces (24 significand bits)", 6, 6.0, "bf16", 0, "k7b_pmc_traffic.json")
                macs = dt_ * P_ * H_ + ((D - dt_) * H_ + nb_ * 2 * H_ * H_ if path == "k8" else 0)
                fp32_flops = 2.0 * B * macs * layers_per_launch
                ach = fp32_flops / (avg_ms * 1e-3) / 1e12
                # HBM: a run of layers reads its rows once and writes them once, and streams every layer's packed weights once
                bytes_ = io_bytes + layers_per_launch * weight_bytes if path == "k8" else (io_bytes + 4 * B * H_) * layers_per_launch
                traffic, traffic_from = load_traffic(traffic_file)
                r = {"bound": "mfma", "kernel": ("nfa::" + ran) if ran else "?",
                     "achieved": ach, "peak": BF16_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": ach / BF16_PEAK_TFLOPS,
                     "traffic": traffic, "traffic_from": traffic_from,
                     "algorithmic_flops_per_launch": fp32_flops,
                     "algorithmic_bytes_per_launch": bytes_,
                     "frac_of_fp32_matrix_peak": ach / 157.3,
                     "matrix_pipe": {"operands": pieces, "products_per_multiply_add": products,
                                     "instruction_time_per_multiply_add_at_the_16_bit_rate": slots,
                                     "executed_flops_per_launch": products * fp32_flops,
                                     "achieved": slots * ach, "unit": "TFLOP/s (16-bit-rate equivalents)",
                                     "frac_of_peak": slots * ach / BF16_PEAK_TFLOPS},
                     "frac_of_hbm_peak_by_survey_bytes": (k1_bytes * layers_per_launch / (avg_ms * 1e-3) / 1e9) / HBM_PEAK_GBS,
                     "note": "achieved = SURVEY 8d's algorithmic flops -- 2 x the fp32 multiply-adds of the layers' GEMMs, "
                             "%d per sample and layer -- / the launch duration; peak = the dense 16-bit MFMA peak of the pipe "
                             "the kernel runs on (the same work against the fp32 matrix peak of 157.3 TFLOP/s: %.2f x).  Every "
                             "fp32 operand is %s and %d cross products per multiply-add run on the %s matrix pipe with fp32 "
                             "accumulation, %.1f instruction times at the 16-bit rate: the pipe was busy for %.0f TFLOP/s of "
                             "16-bit-rate work = %.3f of its peak.  The same launch in SURVEY 8d's "
                             "unfused HBM bytes (3460 B/sample/layer): %.0f GB/s-equivalent of 8000"
                             % (2 * macs, ach / 157.3, pieces, products, pipe, slots, slots * ach,
                                slots * ach / BF16_PEAK_TFLOPS, k1_bytes * layers_per_launch / (avg_ms * 1e-3) / 1e9)}
            elif path == "k7":
                flops = 2.0 * B * H_ * dt_ * P_
                ach = flops / (avg_ms * 1e-3) / 1e12
                r = {"bound": "mfma", "kernel": ("nfa::" + ran) if ran else "nfa::rqs_fused_linear_kernel<false>", "achieved": ach,
                     "peak": 157.3, "unit": "TFLOP/s", "frac": ach / 157.3,
                     "traffic": load_traffic("k7_pmc_traffic.json")[0], "algorithmic_flops_per_launch": flops,
                     "algorithmic_bytes_per_launch": io_bytes + 4 * B * H_}
            else:
                ach = k1_bytes / (avg_ms * 1e-3) / 1e9
                r = {"bound": "hbm", "kernel": ("nfa::" + ran) if ran else "nfa::rqs_coupling_pipelined<8, false, true>", "achieved": ach,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                     "traffic": load_traffic("k1_pmc_traffic.json")[0], "traffic_from": load_traffic("k1_pmc_traffic.json")[1],
                     "algorithmic_bytes_per_launch": k1_bytes}
            r.update(common)
            return r

        roofline = roofline_of(args.path, k1_ms, len(k1_ms) / args.steps, ran=timed_kernel) if k1_ms else None
        if roofline is not None and roofline.get("bound") == "mfma" and not args.skip_mfma_ceiling:
            ceiling = sustained_mfma_ceiling()
            if ceiling and ceiling.get("gaussian_32x32x16"):
                roofline["sustained_mfma_ceiling"] = dict(
                    ceiling, unit="TFLOP/s",
                    note="v_mfma_f32_32x32x16_f16 issued back to back from registers on every SIMD of this box "
                         "(tools/mfma_power_probe.hip), by operand data: with zeros the pipe reaches the spec peak, "
                         "with Gaussian operands the chip's power cap holds it to the `gaussian` figure (clock ~1.75 GHz)")
                roofline["matrix_pipe"]["frac_of_sustained_ceiling"] = roofline["matrix_pipe"]["achieved"] / ceiling["gaussian_32x32x16"]
        roofline_k1 = None
        if args.path != "k1" and not args.skip_k1_roofline and world == 1:  # (N = 1 only: the other ranks are done)
            # the HBM-bound spline kernel K1 (what the fused kernels replace on this shape), measured
            # the same way in a short separate run with the conditioner left to PyTorch / hipBLASLt
            select_path("k1")
            try:
                with torch.no_grad():
                    flow.log_prob(x)
                    torch.cuda.synchronize()
                    _native.check(_native.load().nfa_profile_enable(args.layers * 3))
                    for _ in range(3):
                        flow.log_prob(x)
                    torch.cuda.synchronize()
                    ms = dispatch_durations_ms(args.layers * 3)
                    _native.check(_native.load().nfa_profile_enable(0))
                    k1_ran = ops.last_layer_kernel()
            finally:
                select_path(args.path)
            if ms:
                roofline_k1 = roofline_of("k1", ms, args.layers, ran=k1_ran)
                roofline_k1["note"] = "not in the timed region: PyTorch conditioner + K1 path (--path k1)"
        result = {
            "metric": "log_prob samples/sec (dim=64, K=8, 32-layer RQ-NSF) + max |fwd∘inv − x|",
            "value": total_rows * args.steps / elapsed,
            "unit": "samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "strong" if args.batch_per_gpu is None else "weak",
            "vs_baseline": None,
            # fp32 inputs, outputs, spline arithmetic and accumulation; what the TIMED kernel multiplies in its GEMMs is said here
            "dtype": ({"f16x3": "f32 (inputs, outputs, spline arithmetic, accumulation; conditioner GEMMs: every fp32 operand carried as "
                                "3 f16 pieces = 33 significand bits, i.e. at the reference's own fp32 operand width, 5 cross products per "
                                "multiply-add -- 3 on the f16 MFMA, the 2 at the 2^-22 level from the pieces' high bytes on the bf8 MX "
                                "MFMA --, fp32 accumulate; other_engines_extra: the same step on 2 f16 pieces, "
                                "on 3 bf16 pieces and on fp32 library GEMMs)",
                       "f16x2": "f32 (conditioner GEMMs: each fp32 operand as 2 f16 pieces, 3 cross products on the f16 MFMA pipe, fp32 "
                                "accumulate -- 22-bit operand significands)",
                       "bf16x3": "f32 (conditioner GEMMs: each fp32 operand as 3 bf16 pieces, 6 cross products, fp32 accumulate)"}[args.engine]
                      if args.path == "k8" else
                      "f32 (conditioner GEMMs: each fp32 operand as 3 bf16 pieces, 6 cross products, fp32 accumulate)"
                      if args.path == "k7b" else "f32"),
            "data": "synthetic standard-Gaussian inputs, random-init weights (seed 0)",
            "config": {"workload": "%d-layer RQ-NSF coupling flow (RandomPermutation + RQ coupling, "
                                   "ResidualNet H=128 x2 blocks), dim=64, K=8, tail_bound=3, "
                                   "batch=%d on rank 0 (%s), Flow.log_prob + scalar all-reduce"
                                   % (args.layers, B, "BASELINE configs[3]: 262144 rows over %d GPU%s" % (world, "" if world == 1 else "s")
                                      if args.batch_per_gpu is None else "--batch-per-gpu"),
                       "global_batch": total_rows, "features": D, "num_bins": K, "layers": args.layers,
                       "parallelism": "sample-sharded x%d" % world,
                       "fused_permutations": not args.no_fuse,
                       "engine": args.engine if args.path == "k8" else None,
                       "layer_kernel": {"k8": {"f16x3": "K8x: ResidualNet conditioner (GEMMs on three f16 pieces per operand, five "
                                                        "products) + spline layer in one kernel, the run of layers in one launch",
                                               "f16x2": "K8h: ResidualNet conditioner (GEMMs on two f16 pieces per operand) + spline "
                                                        "layer in one kernel, the run of layers in one launch",
                                               "bf16x3": "K8: ResidualNet conditioner (three bf16 pieces) + spline layer in one kernel, "
                                                         "the run of layers in one launch"}[args.engine],
                                        "k7b": "K7b: final Linear (split-bf16 MFMA) + spline layer",
                                        "k7": "K7: final Linear (fp32 MFMA) + spline layer",
                                        "k1": "PyTorch conditioner + K1 spline layer"}[args.path]},
            "fwd_inv_max_err": {"composite_%d_layers" % args.layers: err_composite, "single_layer": err_layer,
                                "rows": 8192, "composite_stats": err_stats},
            "mean_log_likelihood": mean_ll,
            "redo_blocks": redo_blocks,
            "roofline": roofline,
            "roofline_k1_unfused": roofline_k1,
        }
        if graph_ms is not None:
            result["hip_graph_replay"] = {"ms_per_step": graph_ms, "value": total_rows / (graph_ms * 1e-3),
                                          "note": "same step (incl. copying the batch into the graph's input "
                                                  "buffer) replayed from one captured HIP graph; not the headline"}
        if steady is not None:
            result["steady_state"] = dict(steady, value=total_rows * steady["steps"] / steady["seconds"], unit="samples/s",
                                          note=">= %.1f s of back-to-back steps, same launch path as the timed region"
                                               % args.steady_seconds)
        if other_engines:
            for e in other_engines:
                path_e, engine_e, ms_e, lps_e = e.pop("_roofline_args")
                if ms_e:
                    e["roofline"] = roofline_of(path_e, ms_e, lps_e, ran=e["kernel"], engine=engine_e)
            result["other_engines_extra"] = other_engines
        if fp64_extra is not None:
            result["fwd_inv_max_err"]["fp64_device_path"] = fp64_extra
        if world == 1 and args.batch_per_gpu is None and not args.skip_extra:
            try:
                result["other_configs_extra"] = other_configs(dev, args.steps)
            except Exception as e:  # measurement extra only
                log("other_configs_extra skipped: %r" % (e,))
        if weak is not None:
            result["rows_65536_per_gpu_extra"] = weak
        if small is not None:
            result["small_shards_extra"] = small
        if world == 1 and not args.no_cpu_baseline:
            result["cpu_baseline"] = cpu_baseline(flow_cpu, D, args.cpu_rows,
                                                  x_consistency=None if args.skip_consistency else xs.cpu(),
                                                  full_rows=0 if args.skip_extra else 65536)
            ref_c = result["cpu_baseline"].get("reference_fwd_inv_err_same_rows")
            if ref_c is not None:
                result["fwd_inv_max_err"]["reference_fp32_same_rows"] = ref_c
            result["speedup_vs_cpu_baseline"] = result["value"] / result["cpu_baseline"]["value"]
            if "at_baseline_batch" in result["cpu_baseline"]:
                result["speedup_vs_cpu_baseline_at_65536_rows"] = result["value"] / result["cpu_baseline"]["at_baseline_batch"]["value"]
        print(json.dumps(result))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
