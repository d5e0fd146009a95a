"""The scenario of tests/test_leaf_resolve_blocks_gpu.py (the device) and tests/test_leaf_resolve_blocks_emu.py (the wave emulator):
k_leaf_resolve (csrc/raz_leaf_cache.hip) takes 256 rows per workgroup, counts them with ballots and a prefix over its four waves,
reserves its run of the compact list with one atomic and copies the answers of its hits afterwards.  Slices around that block size
- 1, 3, 4, 5, 255, 256, 257 and 1024 + 1 rows, from row 0 and from row 256 - with rows of every role in every wave of a workgroup,
driven through raz_leaf_cache_probe with the rig and the assertions of tests/leaf_cache_cases.py (check_before: the listed rows are a
permutation of exactly the OWN and PLAIN rows, n_compact plus the served rows are the active rows, the counters are the counts the
rows themselves give; check_after: every active row holds the answer of its position).  No assertion depends on the list's order.

Two parts share one table of 2^12 entries.  Part 1 is a slice of 64 rows behind part 0's.  Row j of part 0's slice, by j % 8:
  0, 6, 7  a position of its own (a fresh claim: OWN)
  1        the position of row j - 1 (a duplicate inside the slice: one of the two is OWN, the other WAIT)
  2        a position part 1 evaluated in an earlier step (ready: HIT)
  3        a position of 30 discs, above max_discs = 24 (PLAIN, never looked up)
  4        inactive
  5        a position a row of part 1 claims in this very round, not yet filled (a duplicate in the OTHER slice: evaluated, PLAIN)"""
import numpy as np

import leaf_cache_cases as C

PNS = (1, 3, 4, 5, 255, 256, 257, 1024 + 1)
P0S = (0, 256)
OTHER = 64                                    # rows of part 1's slice
ROWS = max(P0S) + max(PNS) + OTHER
LOG2, MAX_DISCS = 12, 24


def scenario(run, pn, p0):
    po, pe = C.distinct_homes(max(PNS) + 2 * OTHER + 256, LOG2, seed=8)    # a home slot each: every claim finds room
    keep = C.discs_of(po, pe) <= MAX_DISCS
    po, pe = po[keep], pe[keep]
    assert len(po) >= pn + 2 * OTHER
    ro, re = po[:OTHER], pe[:OTHER]                                    # ready after the first round
    xo, xe = po[OTHER:2 * OTHER], pe[OTHER:2 * OTHER]                  # claimed by part 1 in the second round
    fo, fe = po[2 * OTHER:], pe[2 * OTHER:]
    do, de = C.with_discs(30, 16, 3)
    rig = C.fresh(run, LOG2, ROWS, MAX_DISCS)
    b0 = p0 + pn
    # round 1: part 1 evaluates the positions that are hits later
    rig.own[b0:b0 + OTHER], rig.enemy[b0:b0 + OTHER] = ro, re
    rig.active[:] = 0
    rig.active[b0:b0 + OTHER] = 1
    v = C.one_step(run, rig, b0, OTHER, 1, 1, "poison")
    assert v.kinds(range(b0, b0 + OTHER)) == ["OWN"] * OTHER
    # round 2: part 1 claims (step 2), part 0 runs whole (step 3), part 1 is filled
    j = np.arange(pn)
    cls, k = j % 8, (j // 8) % OTHER
    own, enemy = fo[j].copy(), fe[j].copy()
    own[cls == 1], enemy[cls == 1] = fo[j[cls == 1] - 1], fe[j[cls == 1] - 1]
    own[cls == 2], enemy[cls == 2] = ro[k[cls == 2]], re[k[cls == 2]]
    own[cls == 3], enemy[cls == 3] = do[k[cls == 3] % 16], de[k[cls == 3] % 16]
    own[cls == 5], enemy[cls == 5] = xo[k[cls == 5]], xe[k[cls == 5]]
    rig.own[p0:b0], rig.enemy[p0:b0] = own, enemy
    rig.own[b0:b0 + OTHER], rig.enemy[b0:b0 + OTHER] = xo, xe
    rig.active[:] = 0
    rig.active[p0:b0] = cls != 4
    rig.active[b0:b0 + OTHER] = 1
    other = C.before(run, rig, b0, OTHER, 1, 2)
    assert other.v.kinds(range(b0, b0 + OTHER)) == ["OWN"] * OTHER
    v = C.one_step(run, rig, p0, pn, 0, 3, "poison")
    want = {0: "OWN", 1: "WAIT", 2: "HIT", 3: "PLAIN", 4: "NONE", 5: "PLAIN", 6: "OWN", 7: "OWN"}
    got = v.kinds(range(p0, b0))
    for i, c in enumerate(cls):
        if c == 0 and i + 1 < pn:     # rows i and i + 1 hold one position: either may win the claim, the other waits
            assert sorted(got[i:i + 2]) == ["OWN", "WAIT"], (i, got[i:i + 2])
        elif c != 1:
            assert got[i] == want[c], f"row {p0 + i} (class {c}) is {got[i]}, its position calls for {want[c]}"
    assert int(rig.n_compact[0]) == int(np.isin(cls, (0, 3, 5, 6, 7)).sum())
    C.host_net(rig, other)
    C.after(run, rig, other)
    return v
