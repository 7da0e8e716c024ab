"""Runs a program of Engine.evm_verifier / csrc/evm_codegen.h in the oracle's Yul interpreter (oracle/tools/yul_exec.py, imported
the way tests/golden/make_yul_verdicts.py imports it).  The interpreter is taken as it is; this subclass adds what the generated
programs need beyond the reference's: `calldatasize` over the calldata as sent (the interpreter pads it for its loads), a memory as
large as the program's header says, and - on request - precompile 8 as a true pairing (tests/pairing_ref.py) instead of the
interpreter's shortcut with the seed-0 secret, for programs made under another SRS."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "oracle", "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import yul_exec  # noqa: E402
from zkoracle import curve as C  # noqa: E402

BUILTINS = ("mload mstore mstore8 calldataload calldatasize mulmod addmod add sub mod eq lt and gas keccak256 staticcall revert "
            "return").split()
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47


def header(text):
    """{name: value text} of the `// name: value` lines in front of the object."""
    out = {}
    for ln in text[:text.index("object")].splitlines():
        m = re.match(r"//\s*([^:]+):\s*(.*)$", ln)
        if m:
            out[m.group(1).strip()] = m.group(2).strip()
    return out


def header_cost(text):
    """The header's numbers under the names of zk_evm_cost."""
    h = header(text)
    pre = dict(re.findall(r"(\w+) (\d+)", h["precompile calls"]))
    kc, kb = re.match(r"(\d+) calls, (\d+) bytes", h["keccak256"]).groups()
    return {"calldata_bytes": int(h["calldata bytes"]), "memory_bytes": int(h["memory top"], 16), "modexp": int(pre["modexp"]),
            "ecadd": int(pre["ecAdd"]), "ecmul": int(pre["ecMul"]), "pairing": int(pre["pairing"]), "keccak_calls": int(kc),
            "keccak_bytes": int(kb)}


class VM(yul_exec.VM):
    def __init__(self, calldata, memory_bytes, true_pairing=False):
        super().__init__(calldata)
        self.mem = bytearray(max(memory_bytes, 0x180) + 64)
        self.cd_len = len(calldata)
        self.true_pairing = true_pairing

    def ev(self, e):
        if e[0] == "call" and e[1] == "calldatasize":
            return self.cd_len
        return super().ev(e)

    def _precompile(self, addr, inp, w, ilen, ooff, olen):
        if addr != 8 or not self.true_pairing:
            return super()._precompile(addr, inp, w, ilen, ooff, olen)
        import pairing_ref as pr
        assert ilen == 0x180
        g1 = [self.pt(w(0), w(1)), self.pt(w(6), w(7))]
        g2 = [((w(3), w(2)), (w(5), w(4))), ((w(9), w(8)), (w(11), w(10)))]  # the imaginary part travels first
        assert all(c < Q for pt in g2 for f2 in pt for c in f2)
        f = pr.miller(g1[0], g1[1], pr.prepared_walk(g2[0]), pr.prepared_walk(g2[1]))
        ok = pr.final_exponentiation(f) == pr.F12_ONE
        self.mem[ooff:ooff + olen] = int(ok).to_bytes(32, "big")[:olen]
        return 1


def calldata(instances, proof):
    """snark-verifier's layout (ecdsa_p256.encode_calldata): every instance, circuit-major, as a 32-byte big-endian word; the proof."""
    return b"".join(int(v).to_bytes(32, "big") for vals in instances for v in vals) + bytes(proof)


_parsed = {}


def run(text, data, true_pairing=False):
    """(accepted, vm) of the program on the calldata bytes."""
    if text not in _parsed:
        _parsed.clear()
        _parsed[text] = yul_exec.runtime_block(text)
    vm = VM(data, header_cost(text)["memory_bytes"], true_pairing)
    try:
        vm.run(_parsed[text])
    except yul_exec.Halt as h:
        return (not h.reverted), vm
    return True, vm


def counted(vm):
    """What the run did, under the names of zk_evm_cost (the calls and hashed bytes are the same on every input: the program is
    straight-line and its helpers have no branch)."""
    pc = vm.precompile_calls
    return {"modexp": pc[5], "ecadd": pc[6], "ecmul": pc[7], "pairing": pc[8], "keccak_calls": len(vm.keccak_log),
            "keccak_bytes": sum(n for _, n, _ in vm.keccak_log)}


def called_names(text):
    """(names called, names defined as functions, `not` seen) in the Runtime code."""
    blk = yul_exec.runtime_block(text)
    called, defined = set(), set()

    def expr(e):
        if e[0] == "call":
            called.add(e[1])
            for a in e[2]:
                expr(a)

    def stmt(s):
        k = s[0]
        if k == "block":
            for t in s[1]:
                stmt(t)
        elif k == "func":
            defined.add(s[1])
            stmt(s[4])
        elif k in ("let", "assign"):
            if s[2] is not None:
                expr(s[2])
        elif k == "if":
            expr(s[1])
            stmt(s[2])
        elif k == "expr":
            expr(s[1])

    stmt(blk)
    return called, defined


# ---- the mutations every kind of proof is run through (tests/test_evm_codegen.py, tests/test_gpu_evm_verifier.py) -------------
def mutations(sh, N, scheme, instances, proof):
    """[(name, instances, proof bytes)]: one of each - a byte in each commitment group, an evaluation and an opening point; a
    truncated and an extended calldata; an evaluation + r, an instance + r, a wrong instance value; a coordinate + q, an off-curve
    point, a (0, 0) point.  The instance ones only where there is an instance.  `sh`: a halo2_ref / zkoracle shape."""
    n_pts_c = {"advice": sh.n_adv, "lookup permuted": 2 * sh.n_lookups, "permutation z": sh.n_chunks, "lookup z": sh.n_lookups}
    groups, at = {}, 0
    for name in ("advice", "lookup permuted", "permutation z", "lookup z"):
        groups[name] = at + n_pts_c[name] * (N - 1)  # the last circuit's first point of the group
        at += n_pts_c[name] * N
    groups["random"] = at
    groups["h piece"] = at + 1 + (sh.n_h - 1)
    n_pts = at + 1 + sh.n_h
    n_ev = (len(proof) - 64 * n_pts - 64 * (2 if scheme == "shplonk" else sh.gwc_sets())) // 32
    ev0 = 64 * n_pts
    open0 = ev0 + 32 * n_ev

    def flip(pos, mask=0x10):
        b = bytearray(proof)
        b[pos] ^= mask
        return bytes(b)

    def put(pos, value, size=32):
        b = bytearray(proof)
        b[pos:pos + size] = value.to_bytes(size, "big")
        return bytes(b)

    word = lambda pos: int.from_bytes(proof[pos:pos + 32], "big")
    out = [(name + " commitment", instances, flip(64 * i + 37)) for name, i in groups.items()]
    out.append(("an evaluation", instances, flip(ev0 + 32 * (n_ev // 2) + 20)))
    out.append(("the last opening point", instances, flip(len(proof) - 9)))
    out.append(("truncated", instances, proof[:-32]))
    out.append(("extended", instances, proof + bytes(32)))
    out.append(("an evaluation + r", instances, put(ev0 + 32 * 3, word(ev0 + 32 * 3) + R)))
    out.append(("a coordinate + q", instances, put(64 * 1, word(64 * 1) + Q)))
    out.append(("an off-curve point", instances, put(open0 + 32, (word(open0 + 32) + 1) % Q)))
    out.append(("a (0, 0) point", instances, put(0, 0, 64)))
    if any(len(v) for v in instances):
        c = max(range(N), key=lambda i: len(instances[i]))
        for name, new in (("an instance + r", instances[c][0] + R), ("a wrong instance value", (instances[c][0] + 1) % R)):
            changed = [list(v) for v in instances]
            changed[c][0] = new
            out.append((name, changed, proof))
    return out
