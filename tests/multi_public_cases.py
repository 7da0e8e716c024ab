"""Shared by the tests of the batch and multi forms with public inputs (tests/test_halo2_ref.py,
tests/test_verify_public_forms_host.py, tests/golden/make_multi_public_proofs.py and the tests/test_gpu_*public* files of those
forms): witnesses of ONE key whose instance lists have different lengths, and the lists under which a multi proof must not verify.

One key means one structure: N_PUBLIC gate outputs are tied to instance rows 0 .. N_PUBLIC - 1 in every witness.  A witness whose
list has m < N_PUBLIC values has the other exposed outputs forced to zero (circuit.synthesize's public_values), so that the column
[v_0 .. v_{m-1}, 0, ..] satisfies the copy constraints; a list longer than N_PUBLIC is the full list with zeros appended - the same
column, another transcript."""
import webauthn_halo2_amd as zk
from public_cases import engine_key, mont, params_of
import halo2_ref

N_PUBLIC = 9
WITNESS_SEED = 0x5EED0A00


def witness_with_list(name, lane, m):
    """(assignment, instance list of m values) of lane `lane` (its own witness seed) under the shape's key with N_PUBLIC public inputs."""
    p = params_of(name)
    seed = WITNESS_SEED + 17 * lane
    asg = zk.circuit.synthesize(p, seed, n_public=N_PUBLIC)
    if m >= N_PUBLIC:
        return asg, list(asg.instance) + [0] * (m - N_PUBLIC)
    vals = list(asg.instance[:m]) + [0] * (N_PUBLIC - m)
    return zk.circuit.synthesize(p, seed, n_public=N_PUBLIC, public_values=vals), vals[:m]


def lanes(name, lengths):
    """[(assignment, list)] for the lanes 0 .. with lists of `lengths`; every assignment has the key's structure."""
    return [witness_with_list(name, i, m) for i, m in enumerate(lengths)]


def wrong_multi_lists(lists):
    """[(what, lists)]: per-circuit instance lists under which a multi proof over `lists` must not verify (N >= 2; circuit 1's list
    has a value)."""
    changed = [list(l) for l in lists]
    changed[1][len(changed[1]) // 2] = (changed[1][len(changed[1]) // 2] + 1) % halo2_ref.R
    swapped = [list(l) for l in lists]
    swapped[0], swapped[1] = swapped[1], swapped[0]
    dropped = [list(l) for l in lists]
    dropped[1] = dropped[1][:-1]
    appended = [list(l) for l in lists]
    appended[0] = appended[0] + [0]
    out = [("one changed value in circuit 1's list", changed), ("a dropped value", dropped), ("an appended zero", appended),
           ("one circuit fewer", [list(l) for l in lists[:-1]]), ("one circuit more", [list(l) for l in lists] + [[]])]
    if swapped != [list(l) for l in lists]:
        out.append(("the two circuits' lists swapped", swapped))
    return out


def engine_lanes(eng, name, made, n_inst=1):
    """(pk, advice sets, Montgomery lists) of the lanes `made` (lanes() above) on `eng`: SRS of the shape's k, the key of lane 0's
    structure, every lane's columns resident."""
    pk, sets = engine_key(eng, name, [asg for asg, _ in made], n_inst)
    return pk, sets, [mont(vals) if vals else None for _, vals in made]
