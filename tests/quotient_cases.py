"""Cases for the device harness of csrc/quotient.hip (tests/quotient_device_check.hip, run by tests/test_gpu_quotient_device.py),
their expected rows, and a model of how many terms each lane of each launch accumulates.  No GPU is needed for any of this;
tests/test_quotient_cases.py checks the reference, the model and the coverage of the set on the CPU.

Reference (`reference_rows`).  Plain integers mod r, written from halo2's expressions in halo2's order
(plonk::evaluation::Evaluator::evaluate_h): ONE Horner chain in y over the whole term list, h <- h y + term, one term at a time,
every multiplier (l_0, l_last, l_active) applied inside its own term, rotations as index shifts of 4 r rows on the 4n coset.  It is
not the kernel's grouped form (sums per multiplier, host-made powers of y), and it is not oracle/c/oracle.c orc_quotient, whose
argument layout the kernel shares.  The operations run over numpy object arrays, one element per row: every element is a Python int.
  three cosets   output row j n + r of a C3 launch is the 4n reference at row 4 r + j, j < 3
  accumulating   (previous + row) mod r

Term-count model (`lane_terms`, `folds`).  quotient_row keeps four lazy sums — gate terms, l_0 terms, l_last terms, active-row
terms — and q_acc folds a sum back below 2p at its 32nd term and then every 31 terms (the counter restarts at 1).  The model
restates quotient_log_slices and the launchers' fallback rule (one lane per row when log_slices == 0, N < 256 or N & 255) and gives,
per lane and per sum, the number of terms of a (layout, log_slices, C3) launch.  With C chunks and L lookups over ns lanes:
  gates    the gates j = sl mod ns
  l_0      lane 0's l_0 (1 - z_0), the chunk links c >= 1 with c = sl mod ns, and two terms per lookup l = sl mod ns
  l_last   lane 0's term and one per lookup l = sl mod ns
  active   the chunks c = sl mod ns and two terms per lookup l = sl mod ns
On one lane the l_0 and the active sums both hold C + 2 L terms.

log_slices = 4 cannot fold within MAX_ADV: 16 lanes share at most 352 gates (22 each), at most 176 chunks and 56 lookups
(1 + 10 + 2 * 4 = 19 l_0 terms on lane 0) — every sum stays below 32 terms.  The l_last sum holds at most 1 + 56 terms: one fold.

Case file (32-bit little-endian words): "ZKQC", number of data sets, then per data set
  16 words  log_ext n_gate n_adv n_fix n_perm n_chunks chunk_len n_lookups single last_rot fx_table fx_qlookup has_inst n_vec
            n_launches n_explicit
  fx_sel[n_gate]; perm_src[n_perm] (type << 24 | index; type 0 advice, 1 fixed, 2 instance)
  beta, gamma, y, t_inv[0 .. 3]: 7 x 8 words, canonical integers (t_inv: the honest 1 / ((zeta w_ext^j)^n - 1), or the value
      stored as p - 1)
  n_vec vector records of 17 words in VECTOR ORDER: kind, e0[8], e1[8] (stored words).  kind 1: rows alternate e0 (even), e1 (odd);
      kind 0: explicit, its 2^log_ext rows follow below in record order
  n_explicit x 2^log_ext x 8 words
  n_launches x 4 words: acc, cosets3, divide, log_slices
VECTOR ORDER: adv[n_adv] fix[n_fix] sigma[n_perm] z[n_chunks] lk_z[L] lk_a[L] lk_s[L] inst[has_inst] l0 l_last l_active xs prev.
Every vector is given on the 4n coset; for a three-coset launch the harness lays the rows out coset-major (3 n rows per vector;
the coset points stay in the 4n table, as in the product).  `prev` is what `out` holds before an accumulating launch.
Result file: "ZKQR", number of launches, then per launch (in any order) 4 words (data set, launch, rows, 0) and (256 + rows + 256) x 8 words:
the guard in front of `out`, `out`, the guard behind it.
"""
import itertools
import os
import sys
from dataclasses import dataclass, field as dc_field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
from zkoracle import field as F  # noqa: E402

R = F.R
MONT = F.MONT_R % R
MONT_INV = F.inv(MONT, R)
MAGIC_IN, MAGIC_OUT = 0x43514B5A, 0x52514B5A  # "ZKQC", "ZKQR"
GUARD_ROWS = 256
CANARY = 0xC0DEFACE
MAX_ADV, MAX_FIX, MAX_PERM, MAX_CHUNKS, MAX_LOOKUPS = 352, 304, 352, 176, 56  # csrc/prover.h
BLINDING_FACTORS = 6
LOG_EXTS = (8, 9, 10)
GROUPS = ("gates", "l0", "l_last", "active")
FOLDING = ("gates", "l0", "active")  # the three sums that a legal key can drive past one fold


# ---------------------------------------------------------------------------------------------------------------- layout ---

@dataclass
class Layout:
    """pk.h Layout::init restated: the column layout of a key with A gate columns, L lookup columns, F constants columns, `idle`
    never-enabled gate columns and `inst` instance columns (0 or 1: the last permutation column)."""
    A: int
    L: int
    Fx: int
    idle: int = 0
    inst: int = 0

    def __post_init__(self):
        A, L, Fx, idle = self.A, self.L, self.Fx, self.idle
        assert A >= 1 and L >= 1 and Fx >= 1 and idle < A and 2 * idle <= A and self.inst in (0, 1)
        self.single = A == 1
        self.n_gate = A
        self.n_adv = A + (0 if self.single else L)
        self.fx_table = Fx
        if self.single:
            self.fx_qlookup, fx_sel, self.n_fix = Fx + 1, [Fx + 2], Fx + 3
        else:
            fx_sel = [Fx + 1 + j for j in range(A - idle)] + [None] * idle
            self.fx_qlookup, self.n_fix = 0, Fx + 1 + A - idle
        self.gate_sel = [(c, 0) for c in fx_sel]
        for t in range(0 if self.single else idle):
            self.gate_sel[t] = (fx_sel[t], 1)
            self.gate_sel[A - idle + t] = (fx_sel[t], 2)
        self.perm_cols = [("fixed", f) for f in range(Fx)] + [("advice", j) for j in range(self.n_adv)] + [("instance", 0)] * self.inst
        self.n_perm = len(self.perm_cols)
        self.n_lookups = 1 if self.single else L
        self.chunk_len = 3 if self.single else 2
        self.n_chunks = (self.n_perm + self.chunk_len - 1) // self.chunk_len
        self.last_rot = -(BLINDING_FACTORS + 1)
        self.n_terms = self.n_gate + 2 + (self.n_chunks - 1) + self.n_chunks + 5 * self.n_lookups
        assert self.n_adv <= MAX_ADV and self.n_fix <= MAX_FIX and self.n_perm <= MAX_PERM and self.n_chunks <= MAX_CHUNKS \
            and self.n_lookups <= MAX_LOOKUPS, "outside what zk_keygen accepts"


# ------------------------------------------------------------------------------------------------------ term-count model ---

def quotient_log_slices(log_ext, n_gate, lanes_log=16):
    """quotient.hip quotient_log_slices: lanes per row, as a power of two"""
    ls = 0
    while ls < 4 and log_ext + ls < lanes_log and (2 << ls) <= n_gate:
        ls += 1
    return ls


def launch_rows(log_ext, c3):
    return 3 << (log_ext - 2) if c3 else 1 << log_ext


def effective_log_slices(log_ext, log_slices, c3):
    """the launchers' rule: one lane per row unless the rows fill whole workgroups"""
    N = launch_rows(log_ext, c3)
    return 0 if (log_slices == 0 or N < 256 or (N & 255)) else log_slices


def lane_terms(lay, ns, sl):
    """terms per lazy sum of lane `sl` of `ns` (ns = 1: the one-lane-per-row kernel)"""
    G, C, L = lay.n_gate, lay.n_chunks, lay.n_lookups
    lk = len(range(sl, L, ns))
    links = len(range(1, C)) if ns == 1 else len(range(sl if sl else ns, C, ns))
    first = 1 if sl == 0 else 0
    return {"gates": len(range(sl, G, ns)), "l0": first + links + 2 * lk, "l_last": first + lk, "active": len(range(sl, C, ns)) + 2 * lk}


def fold_positions(count):
    """the terms at which q_acc folds a sum of `count` terms: the 32nd, then every 31st (the counter restarts at 1)"""
    return list(range(32, count + 1, 31))


def folds(count):
    return len(fold_positions(count))


def launch_terms(lay, log_ext, log_slices, c3):
    """per sum, the largest number of terms any lane of the launch accumulates"""
    ns = 1 << effective_log_slices(log_ext, log_slices, c3)
    per = [lane_terms(lay, ns, sl) for sl in range(ns)]
    return {g: max(p[g] for p in per) for g in GROUPS}


def choose_fold_layout(target, exact):
    """The smallest layout whose one-lane sums of gate, l_0 and active-row terms all hold `target` terms (exact) or at least
    `target`, with exactly `target` gates.  C + 2 L = target with C = ceil((F + A + L) / 2) has a solution with F in 1 .. 3 for the
    targets used; otherwise the first layout at or above the target is taken."""
    best = None
    for L, Fx in itertools.product(range(1, MAX_LOOKUPS + 1), (1, 2, 3)):
        try:
            lay = Layout(target, L, Fx)
        except AssertionError:
            continue
        t = lane_terms(lay, 1, 0)
        ok = t["l0"] == target and t["active"] == target if exact else min(t["l0"], t["active"]) >= target
        if ok and (best is None or (t["l0"], L, Fx) < best[0]):
            best = ((t["l0"], L, Fx), lay)
    assert best, "no layout reaches %d terms" % target
    return best[1]


def choose_slice_fold_layout(log_slices):
    """The layout with the fewest gate columns in which the 2^log_slices-lane kernel folds all three sums and goes on adding to
    the folded sum: at least 33 gate terms on every lane, at least 33 l_0 and active-row terms on one (66, 132 and 264 gates for
    2, 4 and 8 lanes)."""
    ns = 1 << log_slices
    for A in range(33 * ns, MAX_ADV + 1):
        for L in range(1, min(MAX_LOOKUPS, MAX_ADV - A) + 1):
            try:
                lay = Layout(A, L, 1)
            except AssertionError:
                continue
            per = [lane_terms(lay, ns, sl) for sl in range(ns)]
            if all(max(p[g] for p in per) >= 33 for g in FOLDING) and min(p["gates"] for p in per) >= 33:
                return lay
    raise AssertionError("no layout folds at log_slices %d" % log_slices)


# ----------------------------------------------------------------------------------------------------------------- cases ---

PM1_WORDS = tuple((R - 1) >> (32 * i) & 0xFFFFFFFF for i in range(8))
ZERO_WORDS = (0,) * 8
ONE_WORDS = tuple(MONT >> (32 * i) & 0xFFFFFFFF for i in range(8))  # the stored form of 1
KINDS = ("max", "zero", "one", "alt", "rand")


@dataclass
class Vec:
    name: str          # "adv", "fix", ...
    index: int
    kind: str          # one of KINDS, or "sel01"
    e0: tuple = ZERO_WORDS
    e1: tuple = ZERO_WORDS
    data: object = None  # explicit: (N, 8) uint32


@dataclass
class Launch:
    acc: int
    c3: int
    divide: int
    log_slices: int


@dataclass
class DataSet:
    name: str
    lay: Layout
    log_ext: int
    round_kind: str    # "allmax", "allrand" or "mixed"
    beta: int
    gamma: int
    y: int
    vecs: list = dc_field(default_factory=list)
    launches: list = dc_field(default_factory=list)
    _ref: dict = dc_field(default_factory=dict)

    @property
    def N(self):
        return 1 << self.log_ext

    def t_inv(self):
        """canonical; honest: 1 / ((zeta w_ext^j)^n - 1) — in the all-(p - 1) round the value whose standard form is p - 1"""
        if self.round_kind == "allmax":
            return [(R - 1) * MONT_INV % R] * 4
        n, w = self.N >> 2, F.omega(self.log_ext)
        return [F.inv((pow(F.ZETA * pow(w, j, R) % R, n, R) - 1) % R, R) for j in range(4)]

    def stored(self, v):
        """the vector's stored words as Python ints, one per row (object array)"""
        if v.data is not None:
            b = np.ascontiguousarray(v.data.astype("<u4")).tobytes()
            return np.array([int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(self.N)], dtype=object)
        e = [sum(w << (32 * i) for i, w in enumerate(x)) for x in (v.e0, v.e1)]
        return np.array([e[i & 1] for i in range(self.N)], dtype=object)

    def values(self, name):
        """the field elements the vectors `name` hold (stored words out of the Montgomery form)"""
        return [self.stored(v) * MONT_INV % R for v in self.vecs if v.name == name]


def vector_order(lay):
    L = lay.n_lookups
    return ([("adv", i) for i in range(lay.n_adv)] + [("fix", i) for i in range(lay.n_fix)] + [("sigma", i) for i in range(lay.n_perm)] +
            [("z", i) for i in range(lay.n_chunks)] + [("lk_z", i) for i in range(L)] + [("lk_a", i) for i in range(L)] +
            [("lk_s", i) for i in range(L)] + [("inst", 0)] * lay.inst + [("l0", 0), ("l_last", 0), ("l_active", 0), ("xs", 0), ("prev", 0)])


WITNESS_SIDE = ("adv", "z", "lk_z", "lk_a", "lk_s", "inst")
KEY_SIDE = ("fix", "sigma", "l0", "l_last", "l_active", "xs")


_R_WORDS = np.array([R >> (32 * i) & 0xFFFFFFFF for i in range(8)], dtype="<u4")


def _rand_rows(rng, N):
    """canonical random elements over the whole range: 254 random bits, and the quarter of them that is not below r cut to 252"""
    v = np.frombuffer(rng.bytes(N * 32), dtype="<u4").reshape(N, 8).copy()
    v[:, 7] &= 0x3FFFFFFF
    below, equal = np.zeros(N, dtype=bool), np.ones(N, dtype=bool)
    for i in range(7, -1, -1):  # v < r, from the top word down
        below |= equal & (v[:, i] < _R_WORDS[i])
        equal &= v[:, i] == _R_WORDS[i]
    v[~below, 7] &= 0x0FFFFFFF
    return v


def make_vec(rng, name, index, kind, N):
    if kind == "max":
        return Vec(name, index, kind, PM1_WORDS, PM1_WORDS)
    if kind == "zero":
        return Vec(name, index, kind, ZERO_WORDS, ZERO_WORDS)
    if kind == "one":
        return Vec(name, index, kind, ONE_WORDS, ONE_WORDS)
    if kind == "alt":
        return Vec(name, index, kind, ZERO_WORDS, PM1_WORDS)  # even rows 0, odd rows p - 1
    if kind == "sel01":  # a selector: 0 or 1 per row
        d = np.zeros((N, 8), dtype="<u4")
        d[rng.integers(0, 2, N).astype(bool)] = np.array(ONE_WORDS, dtype="<u4")
        return Vec(name, index, kind, data=d)
    return Vec(name, index, "rand", data=_rand_rows(rng, N))


def forms_of(lay):
    """every launch form of a layout: plain / ACC, 4n / C3, divide on / off, log_slices 0 .. 4 with 2^log_slices <= n_gate"""
    return [Launch(acc, c3, div, ls) for acc in (0, 1) for c3 in (0, 1) for div in (1, 0) for ls in range(5) if (1 << ls) <= lay.n_gate]


def shapes():
    """(name, layout, sizes, mixed rounds).  The fold shapes come from the model."""
    out = [
        ("single", Layout(1, 1, 1), LOG_EXTS, 3),            # A = 1: q_lookup * adv[0], chunks of three
        ("two_gates", Layout(2, 1, 1), LOG_EXTS, 2),
        ("idle", Layout(5, 2, 2, idle=2), LOG_EXTS, 3),      # selector forms 1, 1, 0, 2, 2
        ("perm7", Layout(4, 2, 1), LOG_EXTS, 2),             # seven permutation columns: the last chunk holds one
        ("inst_joins", Layout(2, 1, 2, inst=1), LOG_EXTS, 2),  # 5 + 1 columns: the instance column fills the third chunk
        ("inst_own", Layout(2, 1, 1, inst=1), LOG_EXTS, 2),    # 4 + 1 columns: a chunk of its own
    ]
    for t in (31, 32, 33):
        out.append(("fold%d" % t, choose_fold_layout(t, True), (8,), 2))
    out.append(("fold63", choose_fold_layout(63, False), (8,), 2))
    out.append(("fold96", choose_fold_layout(96, False), (8,), 2))
    # the widest key zk_keygen accepts (304 fixed columns, 352 permutation columns): nine folds of the gate sum in one lane, eight
    # of the l_0 and active-row sums, one of the l_last sum
    out.append(("widest", Layout(MAX_FIX - 2, MAX_PERM - 1 - (MAX_FIX - 2), 1), (8,), 1))
    for ls in (1, 2, 3):
        # 2^8 rows: the sliced kernel on the 4n route; 2^10 rows: on three cosets too (768 rows; 192 and 384 fall back)
        out.append(("slicefold%d" % ls, choose_slice_fold_layout(ls), (8, 10), 1))
    return out


PRELOADS = ("zero", "max", "rand")


MULTIPLIERS = ("l0", "l_last", "l_active", "xs")  # an all-zero one of these removes a whole group of terms from the row


def build_sets(seed=0x51C0FFEE):
    """Rounds per (shape, size): "allmax" — every stored word p - 1, beta = gamma = y = p - 1 and the stored t_inv p - 1 as well;
    "allrand" — every vector canonical random (the widest spread between the two sides of every subtraction; left out at 2^10
    rows of the slice-fold shapes, whose 1200 vectors would make the case file three times as long); then the mixed rounds —
    every vector one of KINDS at random, the first with every gate selector in {0, 1}.  Mixed and random rounds take honest t_inv
    and challenges of 31 random bytes.  The four multiplier vectors are zero only in the third mixed round of the two smallest
    shapes, one of them per size, so that no other round loses a group of terms."""
    rng = np.random.default_rng(seed)
    sets, turn = [], 0
    for name, lay, sizes, mixed in shapes():
        for log_ext in sizes:
            N = 1 << log_ext
            rounds = ["allmax"] + (["allrand"] if not (name.startswith("slicefold") and log_ext > 8) else []) + ["mixed"] * mixed
            n_mixed = 0
            for round_kind in rounds:
                n_mixed += round_kind == "mixed"
                if round_kind == "allmax":
                    ch = [R - 1] * 3
                else:
                    ch = [int.from_bytes(rng.bytes(31), "little") for _ in range(3)]
                ds = DataSet(name, lay, log_ext, round_kind, *ch)
                zeroed = None
                if n_mixed == 3 and round_kind == "mixed":
                    zeroed = (MULTIPLIERS + (None, None))[LOG_EXTS.index(log_ext) + (0 if name == "single" else 3)]
                for vname, idx in vector_order(lay):
                    if vname == "prev":
                        kind = PRELOADS[len(sets) % 3]
                    elif round_kind == "allmax":
                        kind = "max"
                    elif round_kind == "allrand":
                        kind = "rand"
                    elif vname == "fix" and n_mixed == 1 and any(c == idx for c, _ in lay.gate_sel):
                        kind = "sel01"  # first mixed round: every gate selector in {0, 1}
                    elif vname in MULTIPLIERS:  # one of each kind in turn, a different one for each of the four
                        nonzero = [k for k in KINDS if k != "zero"]
                        kind = "zero" if vname == zeroed else nonzero[(turn + MULTIPLIERS.index(vname)) % len(nonzero)]
                    elif vname == "inst":       # (few of them: in turn as well)
                        kind = KINDS[turn % len(KINDS)]
                    else:
                        kind = KINDS[int(rng.integers(len(KINDS)))]
                    ds.vecs.append(make_vec(rng, vname, idx, kind, N))
                ds.launches = forms_of(lay)
                sets.append(ds)
                turn += round_kind == "mixed"
    return sets


# ------------------------------------------------------------------------------------------------------------- reference ---

def reference_rows(ds):
    """The quotient numerator on the 4n coset, row by row (object array of Python ints): halo2's term list folded as
    h <- h y + term.  The vectors are taken as they stand; nothing here assumes a satisfied circuit."""
    lay, N = ds.lay, ds.N
    beta, gamma, y = ds.beta, ds.gamma, ds.y
    adv, fix, sigma, z = ds.values("adv"), ds.values("fix"), ds.values("sigma"), ds.values("z")
    lk_z, lk_a, lk_s = ds.values("lk_z"), ds.values("lk_a"), ds.values("lk_s")
    inst = ds.values("inst")
    l0, l_last, l_active, xs = (ds.values(k)[0] for k in ("l0", "l_last", "l_active", "xs"))

    def rot(v, r):  # v(w^r X): the extended domain is four times the size of the domain
        return np.roll(v, -4 * r)

    h = np.array([0] * N, dtype=object)

    def term(e):
        nonlocal h
        h = (h * y + e) % R

    # gates: q_j (a_j + a_j(wX) a_j(w^2 X) - a_j(w^3 X)), the selector in its compressed form
    for j in range(lay.n_gate):
        col, form = lay.gate_sel[j]
        q = fix[col]
        if form == 1:
            q = q * (2 - q) % R
        elif form == 2:
            q = q * (1 - q) % R
        a = adv[j]
        term(q * (a + rot(a, 1) * rot(a, 2) - rot(a, 3)) % R)
    # permutation argument
    C, m = lay.n_chunks, lay.chunk_len
    term(l0 * (1 - z[0]) % R)
    term(l_last * (z[C - 1] * z[C - 1] - z[C - 1]) % R)
    for c in range(1, C):
        term(l0 * (z[c] - rot(z[c - 1], lay.last_rot)) % R)
    delta_x = beta * xs % R  # beta delta^p X, p = the column's place in the permutation
    for c in range(C):
        left, right = rot(z[c], 1), z[c]
        for p in range(c * m, min(lay.n_perm, (c + 1) * m)):
            kind, idx = lay.perm_cols[p]
            v = fix[idx] if kind == "fixed" else inst[0] if kind == "instance" else adv[idx]
            left = left * ((v + beta * sigma[p] + gamma) % R) % R
            right = right * ((v + delta_x + gamma) % R) % R
            delta_x = delta_x * F.DELTA % R
        term(l_active * (left - right) % R)
    # lookups
    for l in range(lay.n_lookups):
        inp = fix[lay.fx_qlookup] * adv[0] % R if lay.single else adv[lay.n_gate + l]
        tab = fix[lay.fx_table]
        zl, a, s = lk_z[l], lk_a[l], lk_s[l]
        term(l0 * (1 - zl) % R)
        term(l_last * (zl * zl - zl) % R)
        term(l_active * (rot(zl, 1) * ((a + beta) % R) % R * ((s + gamma) % R) - zl * ((inp + beta) % R) % R * ((tab + gamma) % R)) % R)
        term(l0 * (a - s) % R)
        term(l_active * ((a - s) % R) % R * ((a - rot(a, -1)) % R) % R)
    return h


def _words(ints):
    b = b"".join(int(v).to_bytes(32, "little") for v in ints)
    return np.frombuffer(b, dtype="<u4").reshape(len(ints), 8)


def c3_order(log_ext):
    """4n row of every three-coset row: row j n + r is the point 4 r + j"""
    n = 1 << (log_ext - 2)
    return np.array([4 * r + j for j in range(3) for r in range(n)])


def expected(ds, launch):
    """(rows, 8) uint32: what `out` holds after the launch"""
    key = (launch.acc, launch.c3, launch.divide)
    if key not in ds._ref:
        if "num" not in ds._ref:
            ds._ref["num"] = reference_rows(ds)
            ds._ref["prev"] = ds.values("prev")[0]
        rows = ds._ref["num"]
        if launch.divide:
            ti = ds.t_inv()
            rows = rows * np.array([ti[i & 3] for i in range(ds.N)], dtype=object) % R
        if launch.acc:
            rows = (rows + ds._ref["prev"]) % R
        rows = rows * MONT % R
        if launch.c3:
            rows = rows[c3_order(ds.log_ext)]
        ds._ref[key] = _words(rows)
    return ds._ref[key]


# ------------------------------------------------------------------------------------------------------------------ file ---

def _u32(x):
    return x & 0xFFFFFFFF


def _canon_words(x):
    return [x >> (32 * i) & 0xFFFFFFFF for i in range(8)]


def write_case_file(sets, path):
    with open(path, "wb") as f:
        np.array([MAGIC_IN, len(sets)], dtype="<u4").tofile(f)
        for ds in sets:
            lay = ds.lay
            explicit = [v for v in ds.vecs if v.data is not None]
            hdr = [ds.log_ext, lay.n_gate, lay.n_adv, lay.n_fix, lay.n_perm, lay.n_chunks, lay.chunk_len, lay.n_lookups, int(lay.single),
                   _u32(lay.last_rot), lay.fx_table, lay.fx_qlookup, lay.inst, len(ds.vecs), len(ds.launches), len(explicit)]
            hdr += [c | (form << 24) for c, form in lay.gate_sel]
            hdr += [({"advice": 0, "fixed": 1, "instance": 2}[k] << 24) | i for k, i in lay.perm_cols]
            for c in [ds.beta, ds.gamma, ds.y] + ds.t_inv():
                hdr += _canon_words(c)
            for v in ds.vecs:
                hdr += [0 if v.data is not None else 1] + list(v.e0) + list(v.e1)
            np.array(hdr, dtype="<u4").tofile(f)
            for v in explicit:
                assert v.data.shape == (ds.N, 8)
                v.data.astype("<u4").tofile(f)
            np.array([[l.acc, l.c3, l.divide, l.log_slices] for l in ds.launches], dtype="<u4").tofile(f)


def read_result_file(path, sets):
    """{(data set, launch): (guard before, out rows, guard after)}; asserts the framing and that every launch is there once"""
    raw = np.fromfile(path, dtype="<u4")
    total = sum(len(ds.launches) for ds in sets)
    assert raw[0] == MAGIC_OUT and raw[1] == total, "result file: bad header (%d launches of %d)" % (raw[1], total)
    pos, out = 2, {}
    for _ in range(total):
        si, li, rows, zero = raw[pos:pos + 4].tolist()
        assert si < len(sets) and li < len(sets[si].launches) and (si, li) not in out and zero == 0, "result file: record (%d, %d)" % (si, li)
        assert rows == launch_rows(sets[si].log_ext, sets[si].launches[li].c3), "result file: rows of launch (%d, %d)" % (si, li)
        pos += 4
        blk = raw[pos:pos + (2 * GUARD_ROWS + rows) * 8].reshape(-1, 8)
        pos += blk.size
        out[(si, li)] = (blk[:GUARD_ROWS], blk[GUARD_ROWS:GUARD_ROWS + rows], blk[GUARD_ROWS + rows:])
    assert pos == raw.size, "result file: %d trailing words" % (raw.size - pos)
    return out


# -------------------------------------------------------------------------------------------------------------- coverage ---

def coverage(sets):
    """Which classes of launches the set holds, counted from the layouts, the launch forms and the vector kinds by the model
    alone (no reference value enters)."""
    cls = {}

    def hit(*k):
        cls[k] = cls.get(k, 0) + 1

    for ds in sets:
        lay = ds.lay
        hit("shape", ds.name)
        hit("round", ds.name, ds.round_kind)
        hit("size", ds.name, ds.log_ext)
        if lay.single:
            hit("single_path", ds.round_kind)
        for _, form in lay.gate_sel:
            hit("selector_form", form, ds.round_kind)
        if lay.n_perm % lay.chunk_len == 1:
            hit("last_chunk_holds_one")
        if lay.inst:
            hit("instance", "own_chunk" if (lay.n_perm - 1) % lay.chunk_len == 0 else "joins_chunk")
        for v in ds.vecs:
            side = "witness" if v.name in WITNESS_SIDE else "key" if v.name in KEY_SIDE else "prev"
            hit("operand", side, v.kind)
            hit("operand_of", v.name, v.kind)
        prev = ds.vecs[-1].kind
        for l in ds.launches:
            eff = effective_log_slices(ds.log_ext, l.log_slices, l.c3)
            hit("form", l.acc, l.c3, l.divide, l.log_slices)
            hit("kernel", "sliced" if eff else "rows", l.c3, l.acc)
            hit("kernel_round", "sliced" if eff else "rows", l.c3, l.acc, ds.round_kind)
            if eff:
                hit("sliced_lanes", eff, l.c3)
            if l.c3 and l.log_slices and not eff:
                hit("c3_fallback", ds.log_ext)
            if l.acc:
                hit("acc_preload", prev)
            t = launch_terms(lay, ds.log_ext, l.log_slices, l.c3)
            for g in GROUPS:
                if eff == 0:
                    hit("lane_terms", g, t[g], l.c3, l.acc)
                    hit("lane_folds", g, folds(t[g]), ds.round_kind)
                elif folds(t[g]):
                    hit("slice_folds", eff, g, l.c3, l.acc)
    return cls
