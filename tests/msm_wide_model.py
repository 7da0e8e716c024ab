"""What every buffer of a pass of the wide MSM path (csrc/msm_wide.hip.h) must hold, in plain Python integers — written from the
header's description of the path, not from its kernels — and the two file formats of tests/msm_wide_device_check.hip.

Base points are [a_i] G with known a_i (0: the identity, r - a: the negated point), so every expected group element is [k] G for
a k computed here mod r; the expected points of a pass come from ONE batched cops.fixed_base_g1 call (`Points`).  Device points
are decoded from their limbs (tests/field29_model.py) and compared cross-multiplied: x ZZ = X, y ZZZ = Y, ZZ^3 = ZZZ^2.

The pipeline of a column of n scalars over a table of stride S (window w of base i at index w S + i):
  head    every non-zero signed digit d of window w is an entry (w S + i) | sign in bucket |d| - 1; the entry list is dense and
          sorted by bucket (the order inside a bucket is whatever the atomics gave: never asserted); the first entry of a bucket
          carries WIDE_FLAG and, in bits [ib, 30), min(gap, esc): the empty buckets between it and the previous non-empty bucket
          of its coarse bin (esc = all ones: a bin's first bucket, or a longer gap);
  lanes   lane t sums entries [16 t, 16 t + 16); at a flagged entry (not the lane's first) it stores its sum in slot t + bucket
          and moves to the bucket the distance field names (the escape: the last bucket whose start is <= the position);
  T1      the slots of a bucket are summed into its "heads" among its parts; T2 row and column sums of the bucket matrix
          [nb / 256][256]; T3 the bit sums; the host's Horner gives sum_b (b + 1) B_b.

Case file (32-bit words): MAGIC_IN, bases, geometries; per basis: m, m x 16 words (affine, Montgomery); per geometry: c, S,
max_batch, passes; per pass: basis, n, columns, identity mode (0 unchecked, 1 checked, 2 ask msm_bases_have_identity), T1 mode,
then columns x n x 8 words (Montgomery).  Result file: MAGIC_OUT, records; a record is tag, geometry, pass, column, words, payload
(TAGS below; T_SLOTS / T_PARTS / T_RC hold (index, 36 words) of every element the pass wrote, T_OTHER (kind << 28 | index, value)
of every non-zero word of the counter set the NEXT pass counts in (kind 0 totals, 1 cursors) and of the append cursors (kind 2)).
"""
import random

import numpy as np

from zkoracle import cops, curve, field as F

import field29_model as M

R, P = F.R, F.P
WL, SUB, WCB, LMAX, SUMS = 16, 4096, 512, 24, 20  # entries per lane, entries per sort chunk, bins at most, ZK_T1B_LMAX, sums per column
SIGN, FLAG, NOPART = 1 << 31, 1 << 30, 0xFFFFFFFF
MAGIC_IN, MAGIC_OUT = 0x43574B5A, 0x52574B5A
TAGS = ("geo", "pass", "counts", "totals", "bstart", "pstart", "lane_b", "pbucket", "entries", "sums", "result", "slots", "parts", "rc", "other")
T = {name: i for i, name in enumerate(TAGS)}
STAGES = ("head", "accumulation", "t1", "t2", "t3", "counters")


class Geo:
    """The layout of a wide workspace made for S points at c-bit windows."""

    def __init__(self, c, S):
        self.c, self.S = c, S
        self.nwin, self.nb = 254 // c + 1, 1 << (c - 1)
        self.ib = max(24, (self.nwin * S - 1).bit_length())
        assert 15 <= c <= 17 and self.ib <= 26
        self.fb = min(7, 31 - self.ib)
        self.keys, self.bins = 1 << self.fb, self.nb >> self.fb
        assert self.bins <= WCB
        self.esc = (1 << (30 - self.ib)) - 1
        self.rows = self.nb >> 8
        self.row_bits = self.rows.bit_length() - 1
        self.ent_stride = (S * self.nwin + 63) & ~63
        self.lane_stride = self.ent_stride // WL + 64
        self.slot_stride = self.lane_stride + self.nb + 64
        self.part_stride = ((self.lane_stride + 2 * self.nb) // 2 + self.nb + 2 * self.bins + 127) & ~63
        self.pow2 = [pow(2, c * w, R) for w in range(self.nwin)]


def wcap_for(batch):
    """slots per part: 8 for a lone column and for a batch (ZK_WCAP_ONE, ZK_WCAP_BATCH)"""
    return 8


def slot_count(s, cnt):
    return (s + cnt - 1) // WL - s // WL + 1 if cnt else 0


def digits(s, c):
    """The signed digits of 0 <= s < r in [-2^(c-1), 2^(c-1)), by the carry recoding; equal to the bias recoding."""
    nwin, half = 254 // c + 1, 1 << (c - 1)
    out, carry = [], 0
    for w in range(nwin):
        d = ((s >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 1 if d >= half else 0
        out.append(d - (carry << c))
    assert carry == 0 and sum(d << (c * w) for w, d in enumerate(out)) == s
    K = sum(half << (c * w) for w in range(nwin))
    assert out == [(((s + K) >> (c * w)) & ((1 << c) - 1)) - half for w in range(nwin)]
    return out


def scalar_from_digits(ds, c):
    """A designed scalar: digit ds[w] in window w; the top window stays 0 and the total is positive."""
    nwin = 254 // c + 1
    ds = list(ds) + [0] * (nwin - len(ds))
    assert len(ds) == nwin and ds[-1] == 0 and all(-(1 << (c - 1)) <= d < (1 << (c - 1)) for d in ds)
    s = sum(d << (c * w) for w, d in enumerate(ds))
    assert 0 < s < R and digits(s, c) == ds
    return s


class Column:
    """What the scalars alone fix: the entries of every bucket (as a sorted list), the bucket sums, the MSM."""

    def __init__(self, g, a, scalars):
        self.n = len(scalars)
        self.ents, self.bk, self.msm = {}, {}, 0
        for i, s in enumerate(scalars):
            if s == 0:
                continue
            self.msm = (self.msm + a[i] * s) % R
            for w, d in enumerate(digits(s, g.c)):
                if d:
                    b = abs(d) - 1
                    k = a[i] * g.pow2[w] % R
                    self.ents.setdefault(b, []).append((w * g.S + i) | (SIGN if d < 0 else 0))
                    self.bk[b] = (self.bk.get(b, 0) + (R - k if d < 0 else k)) % R
        self.buckets = sorted(self.ents)
        self.totals = np.zeros(g.nb, dtype=np.int64)
        for b in self.buckets:
            self.ents[b].sort()
            self.totals[b] = len(self.ents[b])
        self.bstart = np.concatenate(([0], np.cumsum(self.totals)[:-1]))
        self.count = int(self.totals.sum())

    def dist(self, g):
        """bucket -> what the distance field of its first entry holds"""
        out, prev = {}, None
        for b in self.buckets:
            out[b] = g.esc if prev is None or prev >> g.fb != b >> g.fb else min(b - prev - 1, g.esc)
            prev = b
        return out

    def slots_of(self, b):
        return slot_count(int(self.bstart[b]), int(self.totals[b]))


# ---------------------------------------------------------------------------------------------- points ---
_FACTOR = {"x29": (1 << 261) % P, "x": (1 << 256) % P, "jac": (1 << 256) % P}  # what a form's stored coordinates are multiplied by


def stored(kind, arr):
    """(X, Y, ZZ, ZZZ) times the form's factor for every row of device words: 36 per row (x29: 4 x 9 limbs of 29 bits, the top
    one longer) or 32 (x: 4 x 8 words); the limbs are joined in 64-bit lanes first, the rest in Python integers"""
    a = np.asarray(arr, dtype=np.uint64)
    if kind == "x29":
        a = a.reshape(-1, 4, 9)
        lanes, step = [a[:, :, 2 * j] + (a[:, :, 2 * j + 1] << np.uint64(29)) for j in range(4)] + [a[:, :, 8]], 58
    else:
        a = a.reshape(-1, 4, 4, 2)
        lanes, step = [a[:, :, j, 0] + (a[:, :, j, 1] << np.uint64(32)) for j in range(4)], 64
    lanes = [l.tolist() for l in lanes]
    return [tuple(sum(l[i][j] << (step * k) for k, l in enumerate(lanes)) % P for j in range(4)) for i in range(a.shape[0])]


def _jac(w):
    ri = pow(_FACTOR["jac"], -1, P)
    X, Y, Z = (M.from_words8([int(v) for v in w[8 * j:8 * j + 8]]) * ri % P for j in range(3))
    return X, Y, Z * Z % P, Z * Z * Z % P


def coords_match(c, m, want):
    """c = (X, Y, ZZ, ZZZ) m: is it `want` (affine, None: the identity)?  Cross-multiplied: x ZZ = X, y ZZZ = Y, ZZ^3 = ZZZ^2"""
    X, Y, ZZ, ZZZ = c
    if want is None:
        return ZZ == 0
    return ZZ != 0 and ZZ * ZZ % P * ZZ % P == ZZZ * ZZZ % P * m % P and want[0] * ZZ % P == X and want[1] * ZZZ % P == Y


def point_matches(kind, w, want):
    return coords_match(_jac(w), 1, want) if kind == "jac" else coords_match(stored(kind, [w])[0], _FACTOR[kind], want)


def affine_of(kind, w):
    X, Y, ZZ, ZZZ = _jac(w) if kind == "jac" else (v * pow(_FACTOR[kind], -1, P) % P for v in stored(kind, [w])[0])
    return None if ZZ == 0 else (X * pow(ZZ, -1, P) % P, Y * pow(ZZZ, -1, P) % P)


def points_of(ks):
    """[k] G for every k, one oracle call"""
    ks = [k % R for k in ks]
    nz = [k for k in ks if k]
    pts = iter(cops.affine_arr_to_ints(cops.fixed_base_g1(cops.fr_mont(nz))) if nz else [])
    return [next(pts) if k else None for k in ks]


class Points:
    """Collects (label, device points, k): the device points must sum to [k] G.  failures() resolves all k in one call."""

    def __init__(self):
        self.items = []

    def add(self, label, kind, words, k):
        self.items.append((label, kind, [words], k))

    def add_sum(self, label, kind, words_list, k):
        self.items.append((label, kind, list(words_list), k))

    def failures(self):
        want = points_of([it[3] for it in self.items])
        ok = [None] * len(self.items)
        for kind in ("x29", "x"):  # the single points of a form, decoded together
            idx = [i for i, it in enumerate(self.items) if it[1] == kind and len(it[2]) == 1]
            if idx:
                for i, c in zip(idx, stored(kind, np.stack([self.items[i][2][0] for i in idx]))):
                    ok[i] = coords_match(c, _FACTOR[kind], want[i])
        bad = []
        for i, (label, kind, ws, _) in enumerate(self.items):
            if ok[i] is None:
                if len(ws) == 1:
                    ok[i] = point_matches(kind, ws[0], want[i])
                else:
                    acc = None
                    for w in ws:
                        acc = curve.add(acc, affine_of(kind, w))
                    ok[i] = acc == want[i]
            if not ok[i]:
                bad.append(label)
        return bad


# ----------------------------------------------------------------------------------------------- dumps ---
class Dump:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _sparse(a, width):
    a = np.asarray(a, dtype=np.uint32).reshape(-1, width + 1)
    return {int(r[0]): r[1:] for r in a}  # (views into the file's array: a dump is a few hundred megabytes)


def parse_results(raw):
    """the result file (a uint32 array) -> {geometry: Dump(info, passes: {pass: Dump(.., cols: {col: Dump})})}"""
    raw = np.asarray(raw, dtype=np.uint32)
    assert raw[0] == MAGIC_OUT, "result file malformed"
    pos, geos = 2, {}
    for _ in range(int(raw[1])):
        tag, gi, pi, q, nw = (int(v) for v in raw[pos:pos + 5])
        body = raw[pos + 5:pos + 5 + nw]
        assert body.size == nw, "result file truncated"
        pos += 5 + nw
        G = geos.setdefault(gi, Dump(info=None, passes={}))
        name = TAGS[tag]
        if name == "geo":
            G.info = Dump(bytes=int(body[0]) | int(body[1]) << 32, ib=int(body[2]), fb=int(body[3]), bins=int(body[4]), rows=int(body[5]),
                          row_bits=int(body[6]), lane_stride=int(body[7]), slot_stride=int(body[8]), part_stride=int(body[9]), wl=int(body[10]),
                          ms=int(body[11]))
            continue
        Pd = G.passes.setdefault(pi, Dump(cols={}, other=[]))
        if name == "pass":
            for k, v in zip(("n", "batch", "may", "t1", "listed", "redone", "counts1", "par", "wcap"), body.tolist()):
                setattr(Pd, k, v)
        elif name == "other":
            Pd.other = [(int(k) >> 28, int(k) & 0xFFFFFFF, int(v)) for k, v in body.reshape(-1, 2)]
        else:
            C = Pd.cols.setdefault(q, Dump())
            setattr(C, name, _sparse(body, 36) if name in ("slots", "parts", "rc") else body.reshape(SUMS, 32) if name == "sums" else body)
    assert pos == raw.size, "result file has trailing words"
    return geos


def records_to_array(records):
    out = [np.array([MAGIC_OUT, len(records)], dtype=np.uint32)]
    for tag, gi, pi, q, body in records:
        body = np.asarray(body, dtype=np.uint32).reshape(-1)
        out += [np.array([T[tag], gi, pi, q, body.size], dtype=np.uint32), body]
    return np.concatenate(out)


# ---------------------------------------------------------------------------------------------- checks ---
def check_head(g, col, d, wcap):
    err = []
    cnt, nparts = int(d.counts[0]), int(d.counts[2])
    if cnt != col.count:
        return ["counts[4 col] = %d, %d non-zero digits" % (cnt, col.count)]
    if not np.array_equal(d.totals, col.totals):
        return ["totals differ at bucket %d" % int(np.nonzero(d.totals != col.totals)[0][0])]
    if not np.array_equal(d.bstart, col.bstart):
        return ["bstart differs at bucket %d" % int(np.nonzero(d.bstart != col.bstart)[0][0])]
    E = d.entries.astype(np.int64)
    if E.size != cnt:
        return ["%d entries dumped, %d counted" % (E.size, cnt)]
    bucket_at = np.repeat(np.arange(g.nb), col.totals)
    key = E & ((1 << g.ib) - 1) | (E & SIGN)
    got = np.lexsort((key, bucket_at))
    want = np.array([e for b in col.buckets for e in col.ents[b]], dtype=np.int64)
    if not np.array_equal(key[got], want):
        bad = int(np.nonzero(key[got] != want)[0][0])
        err.append("the entries of bucket %d are not its digits' (index | sign)" % int(bucket_at[bad]))
    mid_want = np.zeros(cnt, dtype=np.int64)  # bits [ib, 31): the flag and the distance field
    for b, dist in col.dist(g).items():
        mid_want[col.bstart[b]] = (FLAG >> g.ib) | dist
    mid = (E >> g.ib) & ((1 << (31 - g.ib)) - 1)
    for p in np.nonzero(mid != mid_want)[0][:4].tolist():
        b = int(bucket_at[p])
        first = p == col.bstart[b]
        if first and not (E[p] & FLAG):
            err.append("the first entry of bucket %d carries no flag" % b)
        elif first:
            err.append("bucket %d: distance field %d, expected %d" % (b, int(mid[p]) & g.esc, int(mid_want[p]) & g.esc))
        else:
            err.append("entry %d of bucket %d (not its first) has bits [ib, 31) set: %#x" % (p - int(col.bstart[b]), b, int(mid[p])))
    lanes = -(-cnt // WL)
    if d.lane_b.size != lanes or not np.array_equal(d.lane_b, bucket_at[::WL]):
        err.append("lane_b is not the bucket of every lane's first entry")
    if nparts > g.part_stride:
        err.append("counts[4 col + 2] = %d beyond part_stride %d" % (nparts, g.part_stride))
    want_pb = np.full(nparts, NOPART, dtype=np.int64)
    prev_end = 0
    for b in col.buckets:
        p0, npb = int(d.pstart[b]), -(-col.slots_of(b) // wcap)
        if p0 < prev_end or p0 + npb > nparts:
            err.append("bucket %d: parts [%d, %d) overlap the bucket before or leave the list of %d" % (b, p0, p0 + npb, nparts))
            break
        want_pb[p0:p0 + npb] = b
        prev_end = p0 + npb
    else:
        if d.pbucket.size != nparts or not np.array_equal(d.pbucket, want_pb):
            err.append("pbucket is not (bucket of every part, the no-part marker elsewhere)")
    return err


def walk(g, a, d):
    """The accumulation lanes over the DUMPED entries: -> ({slot: k}, errors, per-lane (restarts by distance, by escape),
    lanes that met a step with equal x, lanes whose first entry is flagged)."""
    E, lane_b, bstart = d.entries.tolist(), d.lane_b.tolist(), d.bstart
    mask, slots, err, stats, exc, first_flag = (1 << g.ib) - 1, {}, [], [], [], 0

    def store(t, b, k):
        if t + b in slots:
            err.append("slot %d is written twice" % (t + b))
        slots[t + b] = k

    for t in range(len(lane_b)):
        b, run, cnt, nd, ne, x = lane_b[t], 0, 0, 0, 0, False
        for k, y in enumerate(E[t * WL:(t + 1) * WL]):
            if y & FLAG:
                if k:
                    store(t, b, run)
                    run = cnt = 0
                    dd = (y >> g.ib) & g.esc
                    if dd < g.esc:
                        b, nd = b + 1 + dd, nd + 1
                    else:
                        b, ne = int(np.searchsorted(bstart, t * WL + k, side="right")) - 1, ne + 1
                elif t:
                    first_flag += 1
            w, i = divmod(y & mask, g.S)
            if w >= g.nwin or i >= len(a):
                err.append("entry %d names no table point" % (t * WL + k))
                continue
            q = a[i] * g.pow2[w] % R
            if y & SIGN:
                q = (R - q) % R
            if q == 0:
                continue  # the identity: the checked loop skips it
            if cnt and run and (q == run or q + run == R):
                x = True
            run, cnt = (run + q) % R, cnt + 1
        store(t, b, run)
        stats.append((nd, ne))
        if x:
            exc.append(t)
    return slots, err, stats, exc, first_flag


def check_accumulation(g, a, d, pts, label):
    slots, err, _, exc, _ = walk(g, a, d)
    if set(slots) != set(d.slots):
        miss, extra = sorted(set(slots) - set(d.slots)), sorted(set(d.slots) - set(slots))
        err.append("written slots are not the walk's: %d missing (first %s), %d unexpected (first %s)" % (len(miss), miss[:1], len(extra), extra[:1]))
    for s, k in slots.items():
        if s in d.slots:
            pts.add("%s accumulation: slot %d" % (label, s), "x29", d.slots[s], k)
    return err, bool(exc)


def heads_of(p0, npb):
    return [p0] + list(range((p0 | 63) + 1, p0 + npb, 64))


def check_t1(g, col, d, pts, label, wcap):
    err = []
    for b in col.buckets:
        hs = heads_of(int(d.pstart[b]), -(-col.slots_of(b) // wcap))
        if any(h not in d.parts for h in hs):
            err.append("bucket %d: head %d of its parts was not written" % (b, [h for h in hs if h not in d.parts][0]))
            continue
        pts.add_sum("%s t1: bucket %d" % (label, b), "x29", [d.parts[h] for h in hs], col.bk[b])
    return err


def rowcol(g, col):
    rc = [0] * (g.rows + 256)
    for b, k in col.bk.items():
        rc[b >> 8] = (rc[b >> 8] + k) % R
        rc[g.rows + (b & 255)] = (rc[g.rows + (b & 255)] + k) % R
    return rc


def check_t2(g, col, d, pts, label):
    err = []
    for j, k in enumerate(rowcol(g, col)):
        name = "row %d" % j if j < g.rows else "column %d" % (j - g.rows)
        if j not in d.rc:
            err.append("%s sum was not written" % name)
        else:
            pts.add("%s t2: %s" % (label, name), "x29", d.rc[j], k)
    if set(d.rc) - set(range(g.rows + 256)):
        err.append("row / column sums written beyond rows + 256")
    return err


def bit_sums(g, col):
    rc = rowcol(g, col)
    out = [sum(rc[g.rows + l] for l in range(256) if (l + 1) >> t & 1) % R for t in range(9)]
    return out + [sum(rc[h] for h in range(g.rows) if h >> u & 1) % R for u in range(g.row_bits)]


def check_t3(g, col, d, pts, label):
    ks = bit_sums(g, col)
    # the host's Horner: column sums weigh l + 1, row sums 256 h
    assert (sum(k << t for t, k in enumerate(ks[:9])) + sum(k << (8 + u) for u, k in enumerate(ks[9:]))) % R == col.msm
    for t, k in enumerate(ks):
        pts.add("%s t3: sum %d" % (label, t), "x", d.sums[t], k)
    pts.add("%s t3: collected result" % label, "jac", d.result, col.msm)
    return []


def stage_of(label):
    """the stage a point's label belongs to ("[prefix] column 0 t1: bucket 5")"""
    return label.split(": ")[-2].split(" ")[-1]


def check_pass(g, a, pc, pd, pts=None, prefix="", par=None):
    """Every stage check of one pass: pc = the case (Dump: n, ident, t1, may, cols: lists of scalars), pd = its dump.
    -> {stage: [errors]}.  With a collector `pts` of the caller's (several passes, ONE oracle call) the points are only
    registered, labelled prefix + "column q <stage>: ..."; the caller files pts.failures() by stage_of.  `par`: the counter set
    the NEXT pass must count in (a pass of n > 0 flips it, an empty one counts nothing and flips nothing)."""
    out = {s: [] for s in STAGES}
    own = pts is None
    pts = Points() if own else pts
    wcap = wcap_for(len(pc.cols))
    if (pd.n, pd.batch, pd.t1, pd.may, pd.wcap) != (pc.n, len(pc.cols), pc.t1, int(pc.may), wcap):
        out["head"].append("the pass ran as (n, columns, T1, checked, slots per part) = %s" % ((pd.n, pd.batch, pd.t1, pd.may, pd.wcap),))
    any_exc = False
    for q, scalars in enumerate(pc.cols):
        col, d, label = Column(g, a, scalars), pd.cols[q], "%scolumn %d" % (prefix, q)
        if pc.n:
            out["head"] += ["%s: %s" % (label, e) for e in check_head(g, col, d, wcap)]
            if out["head"]:
                continue  # the later stages are stated over a head that is right
            e, exc = check_accumulation(g, a, d, pts, label)
            any_exc |= exc
            out["accumulation"] += ["%s: %s" % (label, x) for x in e]
            out["t1"] += ["%s: %s" % (label, x) for x in check_t1(g, col, d, pts, label, wcap)]
            out["t2"] += ["%s: %s" % (label, x) for x in check_t2(g, col, d, pts, label)]
        check_t3(g, col, d, pts, label)
    if pc.n and not pc.may and bool(pd.redone) != any_exc and not out["head"]:
        out["accumulation"].append("redone = %d (%d lanes listed), a lane meets equal x: %s" % (pd.redone, pd.listed, any_exc))
    if pc.may and (pd.redone or pd.listed):
        out["accumulation"].append("the checked accumulation listed %d lanes" % pd.listed)
    if par is not None and pd.par != par:
        out["counters"].append("the next pass counts in set %d, expected %d" % (pd.par, par))
    if pd.other:
        out["counters"].append("non-zero after the pass (set, index, value): %s" % (pd.other[:4],))
    if own:
        for label in pts.failures():
            out[stage_of(label)].append(label)
    return out


# ------------------------------------------------------------------------------------------- simulation ---
class Encoder:
    """device encodings of [k] G with arbitrary denominators, all k resolved in one oracle call"""

    def __init__(self, seed):
        self.rng, self.ks, self.pts = random.Random(seed), [], None

    def want(self, k):
        self.ks.append(k)
        return len(self.ks) - 1

    def resolve(self):
        self.pts = points_of(self.ks)

    def x29(self, h):
        pt = self.pts[h]
        if pt is None:
            return [0] * 36
        a = M.lifted(pt, self.rng.randrange(1, P))
        return a.x + a.y + a.zz + a.zzz

    def x(self, h):
        pt, m = self.pts[h], (1 << 256) % P
        if pt is None:
            return M.words8(m) * 2 + [0] * 16
        z = self.rng.randrange(1, P)
        zz, zzz = z * z % P, z * z * z % P
        return sum((M.words8(v * m % P) for v in (pt[0] * zz % P, pt[1] * zzz % P, zz, zzz)), [])

    def jac(self, h):
        pt, m = self.pts[h], (1 << 256) % P
        if pt is None:
            return [0] * 24
        z = self.rng.randrange(1, P)
        return sum((M.words8(v * m % P) for v in (pt[0] * z * z % P, pt[1] * z * z * z % P, z)), [])


def simulate_pass(g, a, pc, gi, pi, order_seed, par, enc):
    """One pass in Python, entries in a seeded arbitrary order inside their buckets -> (the records the harness would write,
    the points still to encode: finish_pass once enc.resolve() has run, the parity after the pass)."""
    rng, wcap, rec, listed, late = random.Random(order_seed), wcap_for(len(pc.cols)), [], 0, []
    for q, scalars in enumerate(pc.cols):
        col = Column(g, a, scalars)
        if pc.n:
            dist, E = col.dist(g), []
            for b in col.buckets:
                es = list(col.ents[b])
                rng.shuffle(es)
                es[0] |= FLAG | dist[b] << g.ib
                E += es
            bucket_at = np.repeat(np.arange(g.nb), col.totals)
            # part regions: per bin (entries / WL + 2 keys) / WCAP rounded up + keys, back to back; buckets consecutive inside
            bin_tot = col.totals.reshape(g.bins, g.keys).sum(axis=1)
            pbase = np.concatenate(([0], np.cumsum([(int(t) // WL + 2 * g.keys + wcap - 1) // wcap + g.keys if t else 0 for t in bin_tot])))
            npb = np.zeros(g.nb, dtype=np.int64)
            for b in col.buckets:
                npb[b] = -(-col.slots_of(b) // wcap)
            before = np.cumsum(npb) - npb
            pstart = np.repeat(pbase[:-1], g.keys) + before - np.repeat(before[::g.keys], g.keys)
            pbucket = np.full(int(pbase[-1]), NOPART, dtype=np.uint32)
            for b in col.buckets:
                pbucket[pstart[b]:pstart[b] + npb[b]] = b
            d = Dump(entries=np.array(E, dtype=np.uint32), lane_b=bucket_at[::WL].astype(np.uint32), bstart=col.bstart.astype(np.uint32))
            slots, err, _, exc, _ = walk(g, a, d)
            assert not err
            listed += 0 if pc.may else len(exc)
            slot_h = {s: enc.want(k) for s, k in slots.items()}
            part_h = {}
            for b in col.buckets:
                ln, p0, n_p = col.slots_of(b), int(pstart[b]), int(npb[b])
                s0 = int(col.bstart[b]) // WL + b
                hs = heads_of(p0, n_p)
                if pc.t1 == 1 and ln <= LMAX:
                    part_h[p0] = enc.want(col.bk[b])
                    for h in hs[1:2]:
                        part_h[h] = enc.want(0)
                    continue
                for j, h in enumerate(hs):
                    end = hs[j + 1] if j + 1 < len(hs) else p0 + n_p
                    lo, hi = s0 + (h - p0) * ln // n_p, s0 + (end - p0) * ln // n_p
                    part_h[h] = enc.want(sum(slots[s] for s in range(lo, hi)))
            rc_h = [enc.want(k) for k in rowcol(g, col)]
            rec += [("counts", gi, pi, q, [col.count, 0, int(pbase[-1])]), ("totals", gi, pi, q, col.totals), ("bstart", gi, pi, q, col.bstart),
                    ("pstart", gi, pi, q, pstart), ("lane_b", gi, pi, q, d.lane_b), ("pbucket", gi, pi, q, pbucket), ("entries", gi, pi, q, d.entries)]
            late += [("slots", gi, pi, q, slot_h), ("parts", gi, pi, q, part_h), ("rc", gi, pi, q, dict(enumerate(rc_h)))]
        late += [("sums", gi, pi, q, [enc.want(k) for k in bit_sums(g, col)]), ("result", gi, pi, q, enc.want(col.msm))]
    par ^= 1 if pc.n else 0
    rec.append(("pass", gi, pi, 0, [pc.n, len(pc.cols), int(pc.may), pc.t1, listed, int(listed > 0), 0, par, wcap]))
    rec.append(("other", gi, pi, 0, []))
    return rec, late, par


def finish_pass(enc, late):
    """the point records of simulate_pass, encoded"""
    rec = []
    for name, gi, pi, q, h in late:
        body = []
        if name == "sums":
            for v in h:
                body += enc.x(v)
            body += (M.words8((1 << 256) % P) * 2 + [0] * 16) * (SUMS - len(h))
        elif name == "result":
            body = enc.jac(h)
        else:
            for i, v in sorted(h.items()):
                body.append(i)
                body += enc.x29(v)
        rec.append((name, gi, pi, q, body))
    return rec
