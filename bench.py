#!/usr/bin/env python
"""bench.py — headline benchmark: WebAuthn ES256 (secp256r1 ECDSA circuit) proofs/sec at k=19.

One "step" = one pass of the create_proof hot path over one job of the k=19 batch workload
(BASELINE.json configs[1] / configs[3]): job i is an independent synthetic witness of seed
0x5eed0019 + i, its advice column resident in HBM when the clock starts.  Rank r of N proves jobs r, r + N,
r + 2N, ... (round-robin, one proof stream per GPU, replicas only — SURVEY.md §8e); the K timed steps of a rank
are K DISTINCT jobs drained through webauthn-halo2_amd/batch.py, so `--gpus 8 --steps 32` IS the 256-proof
batch of configs[3].

Launch: `python bench.py --gpus N ...`.  With N > 1 and no WORLD_SIZE in the environment the script starts its
own N per-device workers (one process per GPU through torch.distributed.run on 127.0.0.1) and relays rank 0's
line — no external launcher needed; launched under torchrun it is a worker.  torch.distributed (RCCL) is used
for the barrier and the max-over-ranks clock only; there is no collective on the data path.

Prints ONE JSON line on rank 0: `value` = proofs/s over exactly K timed steps after the warm-up (W jobs per
pipeline), `ms_per_step` = one timed step.  A plain run does nothing else; `--full` adds, after the timed steps, four
more timed passes, `roofline` for the dominant kernel (HIP events on the engine's own stream), lone-proof latencies,
the k = 17 EVM leg, the comparison of every timed proof with the oracle's committed digests and `cpu_baseline` (a
whole create_proof by the oracle's CPU port on the host cores; the reference Rust prover is not built by this
project).  `--dump-outputs DIR` writes the last timed step's proof.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

K = 19
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
WORKLOAD = ("batch of independent proofs, k=19 (bench_ecdsa.config row 1: A=1,L=1,F=1,lookup_bits=18), Blake2b+SHPLONK, "
            "synthetic same-shape witnesses (job i: seed 0x5eed0019+i, jobs round-robin over ranks and pipelines), one resident "
            "proving key per pipeline; every job's 16 MiB advice column is handed over as a HOST buffer INSIDE the clock (H2D + "
            "canonical -> Montgomery conversion by the pipeline's own thread right before its proof: what a drop-in behind "
            "create_proof receives); `value_advice_resident` is the same batch with the columns in HBM before the clock starts")


SYNTH_PROCESSES = None  # witness pool size (None: batch.py's default); tools/valu_proofs.py sets 1 — rocprofv3 does not survive the pool's workers


def bind_to_gpu_numa_node(device):
    """Bind this rank's host threads (the pipelines' workers, the witness pool) — and therefore the pinned staging buffers they
    allocate — to the NUMA node the GPU hangs off: on an 8-GPU node a rank that proves on GPU 5 from the far socket pays for
    every H2D and every launch.  /sys/bus/pci/devices/<pci id>/{numa_node,local_cpulist}; no-op where the kernel reports no
    node (-1, single-socket boxes).  Returns what was done, for the JSON line."""
    try:
        from webauthn_halo2_amd import engine as E

        pci = E.device_pci_bus_id(device)
        base = "/sys/bus/pci/devices/" + pci
        node = int(open(base + "/numa_node").read().strip())
        cpus = set()
        for part in open(base + "/local_cpulist").read().strip().split(","):
            if part:
                lo, _, hi = part.partition("-")
                cpus.update(range(int(lo), int(hi or lo) + 1))
        cpus &= os.sched_getaffinity(0)
        if node >= 0 and cpus:
            os.sched_setaffinity(0, cpus)
        return {"pci": pci, "numa_node": node, "cpus_bound": len(cpus) if node >= 0 else 0}
    except Exception as e:  # no sysfs entry, no permission: run unbound
        return {"error": str(e)[:80]}


class ProofWorkload:
    """This rank's share of the batch: `inflight` pipelines (own zk_ctx + host thread each) on one GPU, their jobs
    synthesized on the host (process pool) and shipped to HBM before the clock starts."""

    def __init__(self, device, rank, world, inflight, steps, warmup, options=(), lockstep=1, params=None, transcript=None):
        from webauthn_halo2_amd import batch, circuit, engine as E

        made = []

        def configure(e):  # tuning experiments only (--opt id=value -> zk_ctx_set_option right after zk_ctx_create)
            for oid, val in options:
                if isinstance(val, (list, tuple)):  # one value per pipeline, in the order the pipelines are made
                    val = val[len(made) % len(val)]
                e.set_option(oid, val)
            made.append(e)
            return e

        def factory(dev):
            return configure(E.Engine(dev))

        factory.configure = configure

        self.batch, self.E = batch, E
        self.lockstep = max(1, lockstep)
        p = params or circuit.K19
        self.transcript = E.ZK_TRANSCRIPT_BLAKE2B if transcript is None else transcript
        # rank r proves jobs r, r + N, ...: `steps` timed jobs, all distinct (warm-up re-proves the first ones)
        self.jobs = [rank + world * j for j in range(max(steps, 1))]
        self.warm = self.jobs[:max(1, min(len(self.jobs), warmup * inflight))]
        t0 = time.time()
        wit = batch.synthesize_jobs(p, self.jobs, processes=SYNTH_PROCESSES)
        self.synth_s = (time.time() - t0) / len(self.jobs)
        fixed, copies = batch.structure(p)
        t0 = time.time()
        # the further pipelines of this GPU share the first one's resident SRS and window tables (zk_ctx_create_shared)
        self.pipes = []
        for q in range(inflight):
            self.pipes.append(batch.Pipeline(device, p, fixed, copies, engine_factory=factory, deterministic_seeds=True,
                                             share_srs_with=self.pipes[0] if q and not os.environ.get("ZKMI355_BENCH_NO_SHARE") else None))
        self.keygen_s = (time.time() - t0) / inflight
        for q, pl in enumerate(self.pipes):
            for j in self.jobs[q::inflight]:
                pl.load(j, wit[j])
        # the jobs' advice as the host hands it over per request: page-locked staging buffers (zk_host_alloc), filled outside the clock
        self.pinned = {}
        for j in self.jobs:
            bufs = []
            for col in wit[j]:
                pa = E.PinnedArray(col.shape)
                pa.a[...] = col
                bufs.append(pa)
            self.pinned[j] = bufs
            wit[j] = [pa.a for pa in bufs]
        self.wit = wit
        self.host_cols = wit[self.jobs[0]]
        self.engs = [pl.eng for pl in self.pipes]
        self.proofs = {}

    def run(self, jobs):
        """Drain `jobs` over the pipelines (job j lives on pipeline index(j) % inflight)."""
        if self.lockstep > 1:  # every pipeline proves its share `lockstep` jobs at a time (zk_prove_batch)
            self.proofs.update(self.batch.run_lockstep(self.pipes, jobs, self.lockstep, self.transcript, keep=True))
        else:
            self.proofs.update(self.batch.run(self.pipes, jobs, self.transcript, keep=True))
        for e in self.engs:
            e.sync()

    def run_with_h2d(self, jobs):
        """The same drain with every job's advice column shipped from the host INSIDE the clock (16 MiB H2D + the
        canonical -> Montgomery conversion, by the pipeline's own host thread right before its proof — while the other
        pipeline's kernels keep the GPU busy): what a host that hands over host buffers per request sees.  Never `value`."""
        import threading

        out, errs = {}, []

        def work(q):
            # inline, by the pipeline's own host thread right before its proof: 0.4 ms per 16 MiB column, hidden behind the
            # other pipeline's kernels.  Staging job i+1 from a loader thread on its own stream (Pipeline.stage / adopt) was
            # measured slower: tools/stage_timing.py, DESIGN.md
            try:
                pl = self.pipes[q]
                mine = jobs[q::len(self.pipes)]
                for i in range(0, len(mine), self.lockstep):
                    group = mine[i:i + self.lockstep]
                    for j in group:
                        pl.reload(j, self.wit[j])  # into the job's resident buffers: no allocation in the loop
                    if self.lockstep > 1:
                        for j, pf in zip(group, pl.prove_lockstep(group, self.transcript, keep=True)):
                            out[j] = pf
                    else:
                        out[group[0]] = pl.prove(group[0], self.transcript, keep=True)
            except Exception as e:
                errs.append(e)

        ths = [threading.Thread(target=work, args=(q,)) for q in range(len(self.pipes))]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        if errs:
            raise errs[0]
        for e in self.engs:
            e.sync()
        self.proofs.update(out)
        return out

    def single(self):
        """One proof alone on the GPU (single-proof wall clock, the second half of BASELINE.json's metric)."""
        j = self.jobs[0]
        t1 = time.perf_counter()
        self.pipes[0].prove(j, self.transcript, keep=True)
        self.engs[0].sync()
        return (time.perf_counter() - t1) * 1e3

    def single_with_h2d(self):
        """The same with the request's advice column shipped inside the clock (16 MiB H2D + the canonical -> Montgomery
        conversion on the device): what a host that hands over host buffers per request sees.  Never `value`."""
        pl, j = self.pipes[0], self.jobs[0]
        t1 = time.perf_counter()
        pl.reload(j, self.host_cols)
        pl.prove(j, self.transcript, keep=True)
        self.engs[0].sync()
        return (time.perf_counter() - t1) * 1e3

    def close(self):
        for pl in self.pipes:
            pl.close()
        self.wit = None
        for bufs in self.pinned.values():
            for pa in bufs:
                pa.free()


class FakeWorkload:
    """CPU stand-in used only by the gloo tests of the N>1 launch / timing logic (tests/test_multiproc.py):
    no engine, no GPU; a step is a fixed sleep."""

    synth_s = keygen_s = 0.0

    def __init__(self, rank, world, steps):
        self.rank = rank
        self.jobs = [rank + world * j for j in range(steps)]
        self.warm = self.jobs[:1]
        self.proofs = {}

    def run(self, jobs):
        for j in jobs:
            time.sleep(0.01 * (1 + self.rank))
            self.proofs[j] = b"\0" * 960

    def run_with_h2d(self, jobs):
        self.run(jobs)
        return self.proofs

    def close(self):
        pass


def pmc_traffic_bytes(kernel="zk::msm_wacc_fast_kernel"):
    """HBM-side bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes
    (separate FETCH_SIZE / WRITE_SIZE runs of this same command, profiles/*_pmc_hbm.csv; KiB as
    rocprofv3 reports them — on gfx950 FETCH_SIZE under-counts wide coalesced reads 2x, so this is a
    lower bound for streaming reads; the accumulate kernel's reads are 64-byte gathers)."""
    import csv
    import glob

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "*proof_k19_pmc_hbm.csv")))
    if not files:
        return None
    tot = 0.0
    for row in csv.DictReader(open(files[-1])):
        if row["kernel"] == kernel and row["counter"] in ("FETCH_SIZE", "WRITE_SIZE"):
            tot += float(row["avg_value_per_launch"]) * 1024.0
    return tot or None


# Hardware ceiling of the bucket accumulation: the only wide integer multiplier of CDNA4 is v_mad_u64_u32, issued at
# MAD_CYCLES cycles per wave64 instruction per SIMD (tools/ubench_isa.hip on MI355X, profiles/r2_ubench_isa.txt: independent
# mads, 4 waves/SIMD).  One XYZZ mixed addition as the kernel computes it (csrc/ec29.hip.h): 6 products (81 a*b + 81 m*p
# multiply-adds each on the carry-free 9x29-bit form), 2 squarings (45 + 81) and the fused R*(Q - X3) - Y1*PPP (2 x 81 + one
# reduction of 81) = 1 467 multiply-adds; nothing cheaper exists on this ISA (8x32-bit limbs: 128 + carries per product).
MAD_CYCLES = 4.72  # profiles/r6_ubench_isa.txt: v_mad_u64_u32 (indep), 4 waves/SIMD, at the nominal 2.4 GHz the file's "cycles" assume (r2: 4.84)
UBENCH_NOMINAL_GHZ = 2.4  # tools/ubench_isa.hip turns its measured time into "cycles" with hipDeviceProp.clockRate = 2.4 GHz
SIMDS = 1024
MADS_PER_ADD = 6 * 162 + 2 * 126 + 243
# the OTHER vector instructions of a mixed addition as the kernel's text has them (tools/isa_mix.py prints the block: 576 = 285 plain
# VOP2 masks / limb additions, 154 64-bit column shifts and moves, 81 v_mul_lo of the reduction, 56 VOP3 three-operand forms), at
# the rates of profiles/r6_ubench_isa.txt — a plain instruction between two multiply-adds costs 3.96, not the 2.5 of a run of them
OTHER_CYCLES_PER_ADD = 285 * 3.96 + 154 * 4.56 + 81 * 4.3 + 56 * 4.3


def alu_roofline(eng, k, device=0):
    """The dominant kernel against the roofline that actually bounds it: one commitment of a uniformly random column (what 9 of
    the 12 MSMs of a proof are) — bucket additions per second against the issue rate of the chip AT THE CLOCK IT SUSTAINS UNDER
    THIS KERNEL (a probe wave beside the launches: round 5 priced it at a hard-coded 2.4 GHz).  `frac` counts the multiply-adds
    alone (the peak a stream of nothing but v_mad_u64_u32 would reach); `frac_all_instructions` prices the kernel's whole text."""
    import threading

    from webauthn_halo2_amd import engine as E

    n = 1 << k
    rng = np.random.default_rng(0x19)
    col = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    col[:, 3] &= np.uint64((1 << 60) - 1)  # any value < 2^252 < r is a Montgomery image
    p = eng.poly(n, col)
    c, windows = eng.srs_msm_plan()
    eng.commit(p, 1)
    eng.timer_reset()
    ghz = None
    probe = None
    res = {}
    try:
        probe = E.Engine(device)

        def spin():
            time.sleep(0.005)
            res["raw"] = probe.clock_probe(30)

        th = threading.Thread(target=spin)
        th.start()
        t_end = time.perf_counter() + 0.05
        while time.perf_counter() < t_end:  # ~ 45 lone commitments, the probe's 30 ms inside them
            eng.commit(p, 1)  # ZK_BASIS_LAGRANGE
        th.join()
        ghz = res["raw"][0] / max(res["raw"][1], 1) * 0.1
    except Exception:  # noqa: BLE001 — a library without the probe
        for _ in range(5):
            eng.commit(p, 1)
    finally:
        if probe is not None:
            probe.close()
    ms, cnt = eng.timer_stats(4)
    p.free()
    ms /= max(cnt, 1)
    # the rates are TIMES per wave-instruction measured under full VALU load, printed as cycles of the nominal clock: the peak is
    # priced at that same nominal clock (whatever the chip's effective clock was then, it is now); the probe's reading is reported
    clock_ghz = UBENCH_NOMINAL_GHZ
    peak = SIMDS * clock_ghz / MAD_CYCLES * 64 / MADS_PER_ADD
    peak_all = SIMDS * clock_ghz * 64 / (MADS_PER_ADD * MAD_CYCLES + OTHER_CYCLES_PER_ADD)
    adds = n * windows * (1.0 - 2.0 ** -c)  # a signed digit is zero with probability 2^-c
    achieved = adds / (ms * 1e-3) / 1e9
    return {"kernel": "msm_wacc_fast_kernel", "bound": "int-valu (v_mad_u64_u32 issue rate)", "achieved": achieved,
            "peak": peak, "unit": "G mixed adds/s", "frac": achieved / peak, "avg_launch_ms": ms,
            "frac_all_instructions": achieved / peak_all, "peak_all_instructions": peak_all,
            "sclk_ghz_under_this_kernel": ghz, "window_bits": c, "adds_per_launch": adds,
            "peak_model": "%d SIMDs x %.1f GHz (the nominal clock profiles/r6_ubench_isa.txt prints its measured issue times in) / %.2f cycles "
                          "per wave64 v_mad_u64_u32 x 64 lanes / %d mads per mixed add; all instructions: + %.0f issue cycles of non-mad "
                          "instructions per addition"
            % (SIMDS, clock_ghz, MAD_CYCLES, MADS_PER_ADD, OTHER_CYCLES_PER_ADD)}


def kernel_rooflines(eng, pl, wl):
    """The non-dominant kernels against the HBM roofline, each ALONE on the GPU after the timed region (HIP events on the
    engine's stream): SURVEY.md 8(d)'s algorithmic bytes / the solo duration.  All of them are bound by the issue of their integer
    instructions, not by HBM: the fractions say how far."""
    E = wl.E
    n = 1 << K
    N = 4 * n
    rows = []

    def row(kernel, what, alg_bytes, ms):
        gbs = alg_bytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        rows.append({"kernel": kernel, "what": what, "algorithmic_bytes": alg_bytes, "solo_ms": ms, "achieved": gbs, "unit": "GB/s",
                     "frac": gbs / HBM_PEAK_GBS})

    rng = np.random.default_rng(0x21)
    col = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    col[:, 3] &= np.uint64((1 << 60) - 1)
    p, ext = eng.poly(n, col), eng.poly(N)
    for _ in range(2):
        eng.lagrange_to_coeff(p)
    row("ntt_pass_kernel x2", "best_fft 2^19 inverse (lagrange_to_coeff): two passes of 2^10 / 2^9 on 2 048-element tiles", 64.0 * n, eng.last_ms(E.ZK_T_NTT))
    for _ in range(2):
        eng.coeff_to_extended(p, ext)
    row("ntt_pass_kernel x3", "coeff_to_extended 2^19 -> 2^21 (reads n, writes 4n)", 32.0 * (n + N), eng.last_ms(E.ZK_T_NTT))
    for _ in range(2):
        eng.extended_to_coeff(ext, N)
    row("ntt_pass_kernel x3", "best_fft 2^21 inverse on the coset (extended_to_coeff)", 64.0 * N, eng.last_ms(E.ZK_T_NTT))
    eng.timer_reset()
    for _ in range(3):
        eng.commit(p, 1)
    head = (eng.timer_stats(E.ZK_T_MSM)[0] - eng.timer_stats(E.ZK_T_MSM_ACCUM)[0]) / 3
    row("msm_whist + msm_wscatter1 + msm_wfinehist + msm_wscatter2", "MSM sort head of one 2^19 column: 32 B per scalar in, 16 x 4 B entries out",
        96.0 * n, head)
    tail_ms, tail_n = eng.timer_stats(E.ZK_T_MSM_TAIL)
    row("msm_wparts + msm_wrowcol + msm_wbits", "MSM reduction tail of one 2^19 column: 144 B per partial sum (one per lane and bucket)",
        144.0 * (n + 32768), tail_ms / max(tail_n, 1))
    p.free()
    ext.free()
    pl.prove(wl.jobs[0], E.ZK_TRANSCRIPT_BLAKE2B, keep=True)
    row("quotient_kernel", "evaluate_h + division by X^n - 1 at k = 19: 15 extended cosets", 15.0 * N * 32, eng.last_ms(E.ZK_T_QUOTIENT))
    row("poly_eval_batch_kernel", "19 openings of a proof in one launch: 32 B per coefficient and opening", 19.0 * n * 32, eng.last_ms(E.ZK_T_EVAL))
    return rows


def seam_single_proof_ms(eng):
    """What the LITERAL drop-in costs per proof: a Rust host patched at best_multiexp / best_fft only (first
    table) makes 12 MSMs over the resident SRS with host scalars (zk_msm_srs) and 5 + 6 FFTs on host vectors (zk_ntt_bn254_fr at 2^19 /
    2^21) per k = 19 Blake2b proof — every operand crosses PCIe both ways.  Engine time only: the host's own work between the calls
    (transcripts, permutation / lookup provers, quotient on the CPU) comes on top."""
    n = 1 << K
    rng = np.random.default_rng(0x22)
    s = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64)
    s[:, 3] &= np.uint64((1 << 60) - 1)
    big = np.tile(s, (4, 1))
    R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001

    def omega(k):
        w = pow(pow(7, (R - 1) >> 28, R), 1 << (28 - k), R)
        return np.frombuffer(((w << 256) % R).to_bytes(32, "little"), dtype=np.uint64).copy()

    from webauthn_halo2_amd import engine as E

    w19, w21 = omega(K), omega(K + 2)
    a19, a21 = s.copy(), np.ascontiguousarray(big)

    def fft(a, w, log_n):  # in place on the caller's buffer, as best_fft(&mut a, omega, log_n): no copy on the binding's side
        eng._chk(eng.L.zk_ntt_bn254_fr(eng.ctx, E._p(a), E._p(w), log_n), "zk_ntt_bn254_fr")

    eng.msm_srs(s, 1)
    fft(a19, w19, K)
    fft(a21, w21, K + 2)
    t0 = time.perf_counter()
    for i in range(12):
        eng.msm_srs(s, i & 1)
    for _ in range(5):
        fft(a19, w19, K)
    for _ in range(6):
        fft(a21, w21, K + 2)
    return (time.perf_counter() - t0) * 1e3


def cpu_baseline(budget_s=30.0):
    """One WHOLE create_proof on the host cores by the oracle's CPU port (oracle/zkoracle/fastprover.py: the
    reference's algorithms restated — thread-chunked Pippenger best_multiexp for every commitment, radix-2
    best_fft, row-parallel evaluate_h, Horner evaluations, SHPLONK — C kernels under a Python driver), same
    workload shape as the timed GPU steps.  Bounded sample: one k=17 proof (seconds), extrapolated to k=19 only
    if a k=19 proof does not fit the budget."""
    from zkoracle import fastprover

    return fastprover.cpu_baseline(K, budget_s)


def check_against_oracle_digests(proofs):
    """Every timed proof against the committed SHA-256 of the ORACLE's proof of the same job (tests/golden/batch_k19_sha256.json:
    all 256 jobs of BASELINE configs[3], made by the oracle's CPU prover in the build container — data, no oracle code runs
    here).  Returns the number of proofs compared; a mismatch raises."""
    import hashlib

    path = os.path.join(ROOT, "tests", "golden", "batch_k19_sha256.json")
    if not os.path.exists(path):
        return 0
    want = json.load(open(path))["sha256"]
    n = 0
    for j, pf in proofs.items():
        w = want.get(str(j))
        if w is not None:
            if hashlib.sha256(pf).hexdigest() != w:
                raise SystemExit("bench.py: proof of job %d differs from the oracle's (tests/golden/batch_k19_sha256.json)" % j)
            n += 1
    return n


def dump_outputs(path, proof):
    """`--dump-outputs DIR`: what the timed path returned for its last step — one proof — as DIR/proof.npy, its bytes as float32
    values 0..255 (exact).  Jobs and blinding are seeded by the job index, so two builds can be compared byte for byte."""
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "proof.npy"), np.frombuffer(proof, dtype=np.uint8).astype(np.float32))


def digests_on_file(proofs):
    """CPU stand-in of check_against_oracle_digests (the fake workload makes no proofs): how many of this rank's jobs have a
    committed oracle digest to be compared with — `--gpus 8 --steps 32` must find all 256."""
    path = os.path.join(ROOT, "tests", "golden", "batch_k19_sha256.json")
    if not os.path.exists(path):
        return 0
    want = json.load(open(path))["sha256"]
    return sum(1 for j in proofs if str(j) in want)


def _newest(pattern):
    import glob

    files = sorted(glob.glob(os.path.join(ROOT, "profiles", pattern)))
    return files[-1] if files else None


def _kname(k):
    k = k.strip()
    return k[5:] if k.startswith("void ") else k


def clock_under_load(wl, device, jobs):
    """The shader clock the chip sustains WHILE the workload proves (roofline.valu_issue prices the instruction stream in cycles):
    one extra, unreported pass over the timed region's jobs with a probe context beside the pipelines — a single wave that spins
    for 120 ms and reads the shader-clock counter against the constant 100 MHz counter (zk_clock_probe) — and the same probe on
    the idle chip for comparison."""
    import threading

    probe = wl.E.Engine(device)
    res = {}
    try:
        c, r, m = probe.clock_probe(60)
        res["idle_mhz"] = c / max(r, 1) * 100.0

        def spin():
            time.sleep(0.03)  # the pipelines are in their stride
            res["raw"] = probe.clock_probe(120)

        th = threading.Thread(target=spin)
        th.start()
        wl.run_with_h2d(jobs)
        th.join()
        c, r, m = res.pop("raw")
        res["sclk_mhz"] = c / max(r, 1) * 100.0
        res["probe_ms"] = r / 1e5
        res["shader_ticks_per_dependent_mad_lone_wave"] = c / max(m, 1)
        res["how"] = ("zk_clock_probe: s_memtime ticks / s_memrealtime ticks x 100 MHz over 120 ms of one spinning wave, "
                      "on a context of its own while %d pipelines prove (an extra pass after the timed repeats)" % len(wl.pipes))
    finally:
        probe.close()
    return res


def valu_issue_roofline(ms_per_proof, clock):
    """VALU issue as the first-class roofline of this path (round-5 review): none of the kernels is bound by HBM, all of them by
    the issue of their own integer instructions.  Instructions per proof and per kernel = SQ_INSTS_VALU of the committed counter
    pass of this workload (profiles/*_proof_k19_pmc_valu.csv, tools/pmc_valu.sh: the difference of a 5-proof and a 1-proof run);
    a kernel's instructions are priced at the mix-weighted issue TIME of its own text (profiles/*_isa_mix.csv, tools/isa_mix.py):
    the class rates of profiles/r2_ubench_isa.txt are times per wave-instruction per SIMD measured with every SIMD issuing (the
    file prints them as cycles of the nominal 2.4 GHz; the chip's effective clock under such load is whatever it was then and is
    now — the calibration carries it).  floor_ms = the proof's instruction stream at 100 % issue on 1 024 SIMDs; frac = floor_ms /
    measured ms per proof.  The clocks measured in this run (zk_clock_probe) are reported beside it."""
    import csv

    pmc, mix = _newest("*_proof_k19_pmc_valu.csv"), _newest("*_isa_mix.csv")
    if not pmc or not mix:
        return None
    cpi, cpi_mixed = {}, {}
    for r in csv.DictReader(open(mix)):
        cpi[_kname(r["kernel"])] = float(r["issue_cycles_per_valu_instruction"])
        cpi_mixed[_kname(r["kernel"])] = float(r.get("issue_cycles_per_valu_instruction_mixed_stream") or r["issue_cycles_per_valu_instruction"])
    rows, instr, cycles, cycles_mixed, gui, dur = [], 0.0, 0.0, 0.0, 0.0, 0.0
    for r in csv.DictReader(open(pmc)):
        k = _kname(r["kernel"])
        i = float(r["SQ_INSTS_VALU_per_proof"])
        c = cpi.get(k, 2.5)
        instr += i
        cycles += i * c
        cycles_mixed += i * cpi_mixed.get(k, 3.96)
        if "msm_wacc_fast" in k:
            gui, dur = float(r.get("GRBM_GUI_ACTIVE_per_proof", 0) or 0), float(r.get("duration_ns_per_proof_under_the_profiler", 0) or 0)
        rows.append({"kernel": k, "launches_per_proof": float(r["launches_per_proof"]), "instr_per_proof": i,
                     "issue_cycles_per_instr_at_2.4GHz": c, "simd_ns_per_proof": i * c / UBENCH_NOMINAL_GHZ})
    if not instr:
        return None
    for r in rows:
        r["share_of_issue_time"] = r["simd_ns_per_proof"] * UBENCH_NOMINAL_GHZ / cycles
    floor_ms = cycles / UBENCH_NOMINAL_GHZ / SIMDS * 1e-6
    return {"bound": "int-valu issue (wave64 instructions per SIMD)", "instr_per_proof": instr,
            "mix_weighted_ns_per_instr": cycles / instr / UBENCH_NOMINAL_GHZ, "simds": SIMDS,
            "issue_slots_per_s": SIMDS / (cycles / instr / UBENCH_NOMINAL_GHZ * 1e-9), "floor_ms": floor_ms, "ms_per_proof": ms_per_proof,
            "frac": floor_ms / ms_per_proof,
            # the same with plain VOP2 instructions at the 3.96 cycles they cost BETWEEN multiply-adds (r6_ubench_isa.txt "4 mad + 4 v_and")
            # instead of the 2.5 of an uninterrupted run of them: the less optimistic floor
            "floor_ms_mixed_stream": cycles_mixed / UBENCH_NOMINAL_GHZ / SIMDS * 1e-6,
            "frac_mixed_stream": cycles_mixed / UBENCH_NOMINAL_GHZ / SIMDS * 1e-6 / ms_per_proof,
            "sclk_mhz_probe_under_load": (clock or {}).get("sclk_mhz"), "sclk_mhz_probe_idle": (clock or {}).get("idle_mhz"),
            "sclk_mhz_grbm_accumulate_under_profiler": (gui / 8.0 / dur * 1e3) if dur else None,
            "by_kernel": sorted(rows, key=lambda r: -r["simd_ns_per_proof"])[:16],
            "source": "instructions: %s (committed counter pass, NOT this run); class rates: %s + profiles/r2_ubench_isa.txt (times per "
                      "wave-instruction per SIMD, printed there as cycles at the nominal 2.4 GHz); clocks: zk_clock_probe in this run, "
                      "GRBM_GUI_ACTIVE / 8 XCDs / kernel time in the counter pass" % (os.path.basename(pmc), os.path.basename(mix))}


def k17_worker(args):
    """`--k17-worker` (a process of its own, started by rank 0 at N = 1 after the k = 19 figures: a fresh HIP runtime, so that its
    four pipelines get the four hardware queues — DESIGN.md "Streams and hardware queues"): the PROVING SERVER's configuration,
    k = 17 (main.rs:17), EVM transcript + GWC as /prove_evm makes it (main.rs:64-79), 2 720-byte proofs.  `--k17-steps` distinct
    jobs over four pipelines, each job's advice columns handed over as host buffers inside the clock, five timed passes and their
    median; every timed proof compared with the ORACLE's committed digest of that job (tests/golden/batch_k17_evm_sha256.json,
    made by tests/golden/make_batch_hashes.py in the build container)."""
    import hashlib

    from webauthn_halo2_amd import circuit, engine as E

    steps = args.k17_steps
    wl = ProofWorkload(0, 0, 1, max(1, args.inflight), steps, args.warmup, [], 1, params=circuit.K17, transcript=E.ZK_TRANSCRIPT_EVM)
    for _ in range(2):
        wl.run_with_h2d(wl.warm)
    singles = sorted(wl.single() for _ in range(5))
    reps = []
    for _ in range(5):
        wl.proofs.clear()
        for e in wl.engs:
            e.sync()
        t0 = time.perf_counter()
        wl.run_with_h2d(wl.jobs[:steps])
        reps.append(steps / (time.perf_counter() - t0))
    assert len(wl.proofs) == steps and all(len(p) == 2720 for p in wl.proofs.values()) and len(set(wl.proofs.values())) == steps
    path = os.path.join(ROOT, "tests", "golden", "batch_k17_evm_sha256.json")
    want = json.load(open(path))["sha256"] if os.path.exists(path) else {}
    checked = 0
    for j, pf in wl.proofs.items():
        w = want.get(str(j))
        if w is not None:
            if hashlib.sha256(pf).hexdigest() != w:
                raise SystemExit("bench.py: k = 17 EVM proof of job %d differs from the oracle's (tests/golden/batch_k17_evm_sha256.json)" % j)
            checked += 1
    wl.close()
    print(json.dumps({"k17_evm_proofs_per_sec": sorted(reps)[len(reps) // 2], "k17_evm_repeats": reps, "k17_evm_steps": steps,
                      "k17_evm_inflight": len(wl.pipes), "k17_single_proof_evm_ms": singles[len(singles) // 2],
                      "k17_proof_bytes": 2720, "k17_proofs_checked_against_oracle_digests": checked,
                      "k17_config": "bench_ecdsa.config row 3 (A=4, L=1, F=1, lookup_bits=16), EVM transcript + GWC: proving-server/src/main.rs:17,64-79"}))


def k17_leg(args):
    """Runs k17_worker in a fresh process and returns its fields (an error there is reported in the line, never fatal for the headline)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--k17-worker", "--k17-steps", str(args.k17_steps), "--inflight", str(args.inflight),
           "--warmup", str(args.warmup)]
    try:
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT, timeout=600)
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        if out.returncode != 0 or len(lines) != 1:
            return {"k17_error": (out.stderr or out.stdout)[-300:]}
        return json.loads(lines[0])
    except Exception as e:  # noqa: BLE001
        return {"k17_error": str(e)[:300]}


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args, fake):
    """--gpus N > 1 without a launcher: start N per-device workers of this very script (one process per GPU,
    torch.distributed.run, 127.0.0.1 rendezvous) and relay rank 0's JSON line.  N is clamped to the devices that
    exist; the line's n_gpus is the number of workers actually used."""
    n = args.gpus
    if not fake:
        import webauthn_halo2_amd as zk

        have = zk.load_library().zk_device_count()
        if have < 1:
            raise SystemExit("bench.py: no gfx950 device (no CPU fallback exists)")
        if not args.one_device:
            n = min(n, have)
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", str(n), "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--inflight", str(args.inflight), "--lockstep", str(args.lockstep), "--backend", args.backend, "--k17-steps", str(args.k17_steps)]
    cmd += (["--no-cpu-baseline"] if args.no_cpu_baseline else []) + (["--one-device"] if args.one_device else [])
    cmd += (["--full"] if args.full else []) + (["--dump-outputs", os.path.abspath(args.dump_outputs)] if args.dump_outputs else [])
    if n > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
               "--master-port", str(free_port())] + cmd[1:]
    env = dict(os.environ, ZKMI355_BENCH_WORKER="1")
    out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, cwd=ROOT)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    for l in out.stdout.splitlines():
        if not l.startswith("{"):
            print(l, file=sys.stderr)
    if out.returncode != 0 or len(lines) != 1:
        raise SystemExit("bench.py: worker launch failed (rc %d)" % out.returncode)
    print(lines[0])


def full_figures(out, wl, args, world, local_rank, nfl, median):
    """`--full`: every figure of the line beyond the headline, measured after the timed steps (rank 0).  `median`: proofs/s of
    the median timed pass.  Returns the workload, or None once the k = 17 leg has closed it."""
    n = 1 << K
    eng = wl.engs[0]
    acc_total = acc_n = msm_total = msm_n = cols = 0
    for e in wl.engs:
        a, b = e.timer_stats(4)  # ZK_T_MSM_ACCUM
        acc_total, acc_n = acc_total + a, acc_n + b
        a, b = e.timer_stats(0)
        msm_total, msm_n = msm_total + a, msm_n + b
        cols += e.timer_stats(5)[1]  # ZK_T_MSM_COLUMNS: commitments are batched, a launch serves 1-2 columns here
    accum_ms = acc_total / max(acc_n, 1)
    cols_per_launch = cols / max(acc_n, 1)
    alg_bytes = 96.0 * n * cols_per_launch  # MSM(n) = 32 B scalar + 64 B base per point, per column
    achieved = alg_bytes / (accum_ms * 1e-3) / 1e9
    out["roofline"] = {
        "kernel": "msm_wacc_fast_kernel",
        "bound": "hbm",
        "achieved": achieved,
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": achieved / HBM_PEAK_GBS,
        "traffic": pmc_traffic_bytes(),
        "traffic_source": "NOT measured in this run: per-launch FETCH_SIZE + WRITE_SIZE of the committed rocprofv3 PMC passes of "
                          "this same command (latest profiles/*proof_k19_pmc_hbm.csv); hardware counters cannot be read in-process. "
                          "Calibration on the kernel's own access pattern (MI355X_MICROARCH.md, HBM): `traffic_expected` = one 64-byte "
                          "table gather + one 4-byte entry per bucket addition (68 B x 16 x 2^19) + one 144-byte partial sum per lane and "
                          "bucket, per column; the counters report ~88 % of it (part of the 512 MiB table stays in the 256 MiB Infinity "
                          "Cache) — 64-byte gathers are counted at full size, the 2x correction of wide streaming reads does not apply",
        "traffic_expected": (68.0 * 16 * n + 144.0 * (n + 32768)) * cols_per_launch,
        "avg_launch_ms": accum_ms,
        "launches": int(acc_n),
        "columns_per_launch": cols_per_launch,
        "note": "integer-ALU-bound kernel (no MFMA, SURVEY.md 8d); MSM pass, sort .. accumulate, avg %.3f ms x %d per proof as timed inside the overlapping pipelines (reduction tails: on the side stream up to two proofs in flight, on the main stream beyond); quotient kernel %.3f ms"
        % (msm_total / max(msm_n, 1), msm_n // max(args.steps, 1), eng.last_ms(2)),
    }
    out["single_proof_ms"] = sorted(wl.single() for _ in range(5))[2]  # median of five (every latency figure of the line is a median)
    out["roofline"]["alu"] = alu_roofline(eng, K, local_rank)
    try:
        clock = clock_under_load(wl, local_rank, wl.jobs[:args.steps])
    except Exception as e:  # noqa: BLE001 — a library without the probe (A/B variants of older rounds)
        clock = {"error": str(e)[:120]}
    out["roofline"]["clock"] = clock
    out["roofline"]["valu_issue"] = valu_issue_roofline(world / median * 1e3, clock)  # ms per proof on ONE GPU
    # `achieved` above divides by the launches' durations INSIDE the timed region, where the accumulations of the pipelines in
    # flight overlap (each launch shares the chip and takes longer: 0.65 ms with two pipelines on queues that serialised them,
    # ~1.0 ms with four that run side by side — while proofs/s went UP).  The kernel's own rate is the lone launch:
    lone_ms = out["roofline"]["alu"]["avg_launch_ms"]
    out["roofline"]["exclusive"] = {"avg_launch_ms": lone_ms, "columns_per_launch": 1.0, "achieved": 96.0 * n / (lone_ms * 1e-3) / 1e9,
                                    "unit": "GB/s", "frac": 96.0 * n / (lone_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                    "note": "one commitment alone on the GPU after the timed region (same measurement as roofline.alu)"}
    out["roofline"]["launches_overlap"] = ("%d pipelines in flight: their accumulate launches overlap in time, so the per-launch "
                                           "duration of the timed region (and of the rocprofv3 summary of this command) is not the "
                                           "kernel's own rate — see `exclusive`" % nfl)
    # BASELINE.json configs[2]: the same proof with the EVM (Keccak) transcript and GWC, as /prove_evm makes it
    pl = wl.pipes[0]
    evm = []
    for i in range(5):
        t1 = time.perf_counter()
        pe = pl.eng.prove(pl.pk, pl.resident[wl.jobs[0]], bytes([i + 1]) * 32, wl.E.ZK_TRANSCRIPT_EVM)
        evm.append(time.perf_counter() - t1)
    assert len(pe) == 1536
    out["single_proof_evm_ms"] = sorted(evm)[2] * 1e3  # median of five, like single_proof_ms (round 5: a minimum of three)
    out["single_proof_with_h2d_ms"] = sorted(wl.single_with_h2d() for _ in range(5))[2]  # PCIe-inclusive; never `value`
    out["roofline"]["kernels"] = kernel_rooflines(eng, pl, wl)
    out["single_proof_seam_ms"] = seam_single_proof_ms(eng)
    if world == 1 and args.k17_steps > 0:
        # BASELINE.json configs[0]'s degree and the proving server's own (main.rs:17): k = 17, here as /prove_evm makes it
        wl.close()
        wl = None
        out.update(k17_leg(args))
    if world == 1 and not args.no_cpu_baseline:
        cb = cpu_baseline()
        out["cpu_baseline_k17"] = cb.pop("k17", None)  # configs[0]: bench_secp256r1_ecdsa at k = 17, Blake2b, CPU only
        out["cpu_baseline"] = cb
    return wl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--inflight", type=int, default=4,
                    help="independent proof pipelines per GPU (each its own zk_ctx + host thread); the K timed steps are "
                         "shared among them.  1 = strictly one proof at a time (single-proof latency).  4 = one pipeline per "
                         "hardware queue of the HIP runtime: with three or more proofs in flight the engine keeps every "
                         "pipeline on ONE stream (round 4: 94 -> 102-104 proofs/s; 5 pipelines share queues again: 96)")
    ap.add_argument("--lockstep", type=int, default=1,
                    help="proofs a pipeline advances together (zk_prove_batch: the same commitment of all of them in one MSM pass, "
                         "the same transform in one NTT launch); 1 = one zk_prove per job")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="torch.distributed backend of the barrier and the clock reduction (gloo: CPU tensors — ranks that share a device)")
    ap.add_argument("--one-device", action="store_true",
                    help="every rank proves on device 0 (tests/test_gpu_torchrun.py: two worker processes on ONE GPU, the N > 1 path on hardware)")
    ap.add_argument("--k17-steps", type=int, default=40,
                    help="jobs of the k = 17 EVM + GWC leg (the proving server's configuration, main.rs:17,64-79), 0 = skip; N = 1 only")
    ap.add_argument("--k17-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--opt", action="append", default=[], metavar="ID=VALUE",
                    help="tuning experiments: zk_ctx_set_option(ID, VALUE) on every pipeline (include/zkmi355.h ZK_OPT_*)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline, after the timed steps: four more timed passes (median and spread), "
                         "the resident-advice pass, lone-proof latencies, rooflines, the seam figure, the k = 17 EVM leg, the CPU "
                         "baseline and the comparison of every timed proof with the oracle's committed digests")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the proof of the last timed step (rank 0) to DIR/proof.npy: its bytes as float32 values 0..255")
    args = ap.parse_args()
    options = []
    for o in args.opt:  # ID=VALUE, or ID=V0,V1,.. (one value per pipeline)
        oid, val = o.split("=")
        vals = [int(x) for x in val.split(",")]
        options.append((int(oid), vals[0] if len(vals) == 1 else vals))

    if args.k17_worker:
        return k17_worker(args)
    fake = os.environ.get("ZKMI355_BENCH_FAKE") == "1"  # CPU test of the launch/timing logic only
    if "WORLD_SIZE" not in os.environ and args.gpus > 1 and os.environ.get("ZKMI355_BENCH_WORKER") != "1":
        return self_launch(args, fake)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    torch = None
    if world > 1 or "RANK" in os.environ:  # launched by torchrun (also with one rank: the same barrier / reduce path runs)
        import torch
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if fake or args.backend == "gloo":
            dist.init_process_group(backend="gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    cpu_tensors = fake or args.backend == "gloo"  # gloo: the clock and the job lists travel as CPU tensors (ranks may share a device)
    tdev = "cpu" if cpu_tensors else "cuda"
    if args.one_device:
        local_rank = 0

    nfl = max(1, args.inflight)
    numa = None if fake else bind_to_gpu_numa_node(local_rank)
    if fake:
        wl = FakeWorkload(rank, world, args.steps)
    else:
        # independent proof streams: replicas, no data-path collective.  `inflight` pipelines share one GPU so
        # that the latency-bound phases of one proof (transcript round trips, reduction tails) overlap the
        # throughput-bound kernels of another.
        wl = ProofWorkload(local_rank, rank, world, nfl, args.steps, args.warmup, options, args.lockstep)

    def barrier():
        if not fake:
            for e in wl.engs:
                e.sync()
        if dist is not None:
            if not cpu_tensors:
                torch.cuda.synchronize()
            dist.barrier()
            if not cpu_tensors:
                torch.cuda.synchronize()

    for _ in range(1 if fake else max(1, (args.warmup * nfl + len(wl.warm) - 1) // len(wl.warm))):
        wl.run_with_h2d(wl.warm)  # the timed region's own path: upload from the pinned staging buffer, then prove
    if not fake:
        for e in wl.engs:
            e.timer_reset()
    wl.proofs.clear()
    barrier()
    t0 = time.perf_counter()
    wl.run_with_h2d(wl.jobs[:args.steps])  # EXACTLY K steps on this rank: K distinct jobs, each job's advice shipped inside the clock
    barrier()
    elapsed = time.perf_counter() - t0
    assert len(wl.proofs) == args.steps
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, wl.proofs[wl.jobs[args.steps - 1]])
    per_rank_ms = [elapsed / args.steps * 1e3]
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=tdev)
        every = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(every, t)  # every rank's own clock: a SCALE record can show imbalance between replicas
        per_rank_ms = [float(x.item()) / args.steps * 1e3 for x in every]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    host_setup = {"synthesize_s_per_job": round(wl.synth_s, 3), "keygen_s": round(wl.keygen_s, 3)}
    if dist is not None:
        # every rank's set-up time (SRS + window tables + key + workspaces, per pipeline): a SCALE record separates it from steady state
        ks = torch.tensor([wl.keygen_s], dtype=torch.float64, device=tdev)
        allk = [torch.zeros_like(ks) for _ in range(world)]
        dist.all_gather(allk, ks)
        host_setup["keygen_s_per_rank"] = [round(float(x.item()), 3) for x in allk]
    # which jobs of the batch were proved, over all ranks: `--gpus 8 --steps 32` must cover the 256 jobs of configs[3] exactly once
    mine = list(wl.jobs[:args.steps])
    covered = sorted(mine)
    if dist is not None:
        tj = torch.tensor(mine, dtype=torch.int64, device=tdev)
        allj = [torch.zeros_like(tj) for _ in range(world)]
        dist.all_gather(allj, tj)
        covered = sorted(int(x) for t_ in allj for x in t_.tolist())
    jobs_exactly_once = covered == list(range(world * args.steps))
    assert jobs_exactly_once, "the ranks' jobs do not partition 0 .. world x steps - 1"
    launcher = {"launcher": "torchrun" if dist is not None else "in-process", "jobs_covered_exactly_once": jobs_exactly_once,
                "ranks_share_device": bool(args.one_device and world > 1),
                "numa_binding": numa,
                "dist_backend": (dist.get_backend() if dist is not None else None), "ms_per_step_per_rank": per_rank_ms}
    value = world * args.steps / elapsed

    if args.full:
        # byte parity of the timed steps themselves: every rank compares its proofs with the oracle's digests (outside the clock)
        oracle_checked = digests_on_file(wl.proofs) if fake else check_against_oracle_digests(wl.proofs)
        if dist is not None:
            tc = torch.tensor([oracle_checked], dtype=torch.float64, device=tdev)
            dist.all_reduce(tc, op=dist.ReduceOp.SUM)
            oracle_checked = int(tc.item())
        # timed proofs (all ranks) whose bytes were compared with the oracle's committed digests: all of them for the 256-job batch
        # of configs[3]
        launcher["proofs_checked_against_oracle_digests"] = oracle_checked

        pass_ranks = [per_rank_ms]  # every timed pass's per-rank clocks

        def timed(fn, record=True):
            """One more timed pass over the same K jobs (same barriers, max-over-ranks clock) -> whole-job proofs/s."""
            barrier()
            t1 = time.perf_counter()
            fn(wl.jobs[:args.steps])
            barrier()
            dt = time.perf_counter() - t1
            mine_ms = [dt / args.steps * 1e3]
            if dist is not None:
                tt = torch.tensor([dt], dtype=torch.float64, device=tdev)
                ev = [torch.zeros_like(tt) for _ in range(world)]
                dist.all_gather(ev, tt)
                mine_ms = [float(x.item()) / args.steps * 1e3 for x in ev]
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                dt = float(tt.item())
            if record:
                pass_ranks.append(mine_ms)
            return world * args.steps / dt

        # Four further timed repeats of the same region (after `value`'s): the median and the spread say how large a
        # round-over-round delta must be before it means anything (boxes and runs differ by ~3 %).  `value_median` is what
        # round 6 reported as `value`.
        repeats = [value] + [timed(wl.run_with_h2d) for _ in range(0 if fake else 4)]
        median = sorted(repeats)[len(repeats) // 2]
        launcher["ms_per_step_per_rank_median"] = pass_ranks[repeats.index(median)]
        launcher["value_first"] = repeats[0]
        launcher["value_repeats"] = repeats
        launcher["value_median"] = median
        launcher["value_spread_pct"] = (max(repeats) - min(repeats)) / (sum(repeats) / len(repeats)) * 100.0
        if not fake:
            launcher["value_advice_resident"] = timed(wl.run, record=False)  # the columns already in HBM (rounds 1-4 reported this as `value`)

    if rank == 0 and fake:
        print(json.dumps({"metric": "webauthn_es256_proofs_per_sec_k19", "value": value,
                          "unit": "proofs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": world / value * 1e3, "scaling": "weak", "data": "fake",
                          "jobs_total": world * args.steps, "host_setup": host_setup, **launcher}))
    elif rank == 0:
        assert all(len(p) == 960 for p in wl.proofs.values())  # halo2-circuits/src/results/ecdsa_bench.csv:2
        assert len(set(wl.proofs.values())) == len(wl.proofs)  # distinct jobs -> distinct proofs: nothing cached
        out = {
            "metric": "webauthn_es256_proofs_per_sec_k19",
            "value": value,
            "unit": "proofs/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": world / value * 1e3,  # of the K timed steps
            **launcher,
            "inflight_per_gpu": nfl,
            "lockstep": args.lockstep,
            "jobs_total": world * args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # BASELINE.json "published" is {}: the only reference number (14.846 s/proof, M1 Pro, README.md:38) is other hardware
            "host_setup": host_setup,
            "dtype": "u256-montgomery (9x29-bit carry-free limbs in the hot kernels: bucket accumulation, NTT, reduction tails, quotient; 8x32-bit limbs elsewhere and in memory)",
            "data": "synthetic",
            "config": {"workload": WORKLOAD, "k": K, "transcript": "blake2b", "multiopen": "shplonk", "proof_bytes": 960,
                       "parallelism": "replicas:%d (one independent proof stream per GPU, no collective)" % world},
        }
        if args.full:
            wl = full_figures(out, wl, args, world, local_rank, nfl, launcher["value_median"])
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if wl is not None:
        wl.close()


if __name__ == "__main__":
    main()
