"""Inputs, numpy restatements and assertions for the evaluation cache's three kernels - k_leaf_claim, k_leaf_resolve, k_leaf_fill of
csrc/raz_leaf_cache.hip - row by row, through raz_leaf_cache_probe (include/raz.h).  Shared by tests/test_leaf_cache_gpu.py (the device)
and tests/test_leaf_cache_emu.py (the wave emulator); a scenario takes `run(rig, calls, **overrides) -> [status codes]`, which executes
a list of (phase, p0, pn, part, step) calls back to back on the arrays of a Rig and leaves their results in those arrays, and knows
nothing of where the kernels execute.

The whole-game tests of the cache prove that games do not change.  They cannot reach the guards that make a served answer the answer of
THAT position - the key comparison after a tag match, the stamp and owner-in-this-slice comparisons, the 8-probe window and its wrap,
the disc threshold, the slice-relative list - because played positions never share a tag and no game leaves a claim unfinished.  The
inputs here are built for those guards: pairs of positions with one tag (leaf_tag's finalizer run backwards), groups of positions with
one home slot, claims without a fill, the same positions in two slices.

Restated here, independently of the kernels: leaf_tag, the home slot, the byte layout of the buffer.  The "net" is a pure function of
the position (`net`), so what a row or an entry must hold is known without a net.  Every comparison is of integers or bit patterns, and
none depends on which thread wins a race: where two rows of one position compete, either may own the entry."""
import functools

import numpy as np

RAZ_EINVAL = -1
CLEAR, BEFORE, AFTER = 0, 1, 2
NONE, PLAIN, OWN, FOLLOW, WAIT = range(5)        # role & 7 (csrc/raz_leaf_cache.hip); role >> 3 = the entry
PROBES = 8
POISON = 0xdeadbeef
MODES = ("poison", "prefilled")
U = np.uint64
K1, K2, K3 = 0x9E3779B97F4A7C15, 0xD6E8FEB86659FD93, 0xC2B2AE3D27D4EB4F
M1, M2 = 0xFF51AFD7ED558CCD, 0xC4CEB9FE1A85EC53
MASK64 = (1 << 64) - 1
INIT_OWN, INIT_ENEMY = 0x0000000810000000, 0x0000001008000000


def _rng(tag):
    return np.random.default_rng([20250311, tag])


def _u(x):
    return np.atleast_1d(np.asarray(x, dtype=np.uint64))


# ---------------------------------------------------------------------------------------------------------------- the hash, restated
def _fin(x):
    """leaf_tag's finalizer on uint64 arrays (numpy's array arithmetic wraps around, as the device's does)."""
    x = x ^ (x >> U(32))
    x = x * U(M1)
    x = x ^ (x >> U(29))
    x = x * U(M2)
    return x ^ (x >> U(32))


def pre_tag(own, enemy):
    own, enemy = _u(own), _u(enemy)
    return _fin((own * U(K1)) ^ ((enemy + U(K2)) * U(K3)))


def leaf_tag(own, enemy):
    return pre_tag(own, enemy) | U(1)


def home_slot(tag, log2_entries):
    return ((_u(tag) >> U(24)) & U((1 << log2_entries) - 1)).astype(np.int64)


def discs_of(own, enemy):
    x = np.ascontiguousarray(_u(own) | _u(enemy))
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)


def _fin_int(x):
    x ^= x >> 32
    x = x * M1 & MASK64
    x ^= x >> 29
    x = x * M2 & MASK64
    return x ^ (x >> 32)


def _unfin_int(y):
    """_fin backwards: x ^= x >> 32 is its own inverse, x ^= x >> 29 is undone by y ^ y >> 29 ^ y >> 58, the multipliers are odd."""
    y ^= y >> 32
    y = y * pow(M2, -1, 1 << 64) & MASK64
    y ^= (y >> 29) ^ (y >> 58)
    y = y * pow(M1, -1, 1 << 64) & MASK64
    return y ^ (y >> 32)


def net(own, enemy):
    """The synthetic net: uint32[n][65] - the bit patterns of 64 finite float32 policy values and one value, every one taken from a
    64-bit hash of (own, enemy, k), so that two positions share no number (up to the chance of two equal 32-bit hashes, which no
    assertion relies on: rows are compared whole)."""
    own, enemy = _u(own)[:, None], _u(enemy)[:, None]
    k = np.arange(1, 66, dtype=np.uint64)[None, :]
    h = _fin(_fin(own + k * U(K3)) ^ (enemy * U(K1)) ^ (k << U(56)))
    w = (h >> U(32)).astype(np.uint32)
    e = np.clip((w >> np.uint32(23)) & np.uint32(0xff), 1, 254).astype(np.uint32)   # exponent 1..254: finite, not subnormal
    return (w & np.uint32(0x807fffff)) | (e << np.uint32(23))


# ---------------------------------------------------------------------------------------------------------------- the buffer, restated
def sections(log2_entries, rows):
    """{name: (offset, bytes)} and the total: tags, keys, stamp, owner, ready, pv, counters, n_compact, list, role, each rounded up to
    256 bytes (include/raz.h raz_leaf_cache_probe)."""
    E = 1 << log2_entries
    sizes = [("tags", E * 8), ("keys", E * 16), ("stamp", E * 4), ("owner", E * 4), ("ready", E * 4), ("pv", E * 72 * 4),
             ("counters", 8 * 8), ("n_compact", 16 * 4), ("list", rows * 4), ("role", rows * 4)]
    off, out = 0, {}
    for name, n in sizes:
        out[name] = (off, n)
        off = (off + n + 255) // 256 * 256
    return out, off


def check_layout(bytes_of):
    """bytes_of = raz_leaf_cache_bytes."""
    for log2 in (10, 11):
        for rows in (1, 63, 64, 65, 600):
            assert bytes_of(log2, rows) == sections(log2, rows)[1], (log2, rows)
    assert bytes_of(9, 64) == 0 and bytes_of(29, 64) == 0


_DTYPES = {"tags": np.uint64, "keys": np.uint64, "counters": np.uint64}


class Rig:
    """The host image of everything a probe call touches: the cache buffer (256-byte aligned, with named views of its sections) and the
    rows' own / enemy / active / policy / value.  policy, value and pv are kept as uint32 bit patterns.  A new buffer holds garbage,
    not zeros: clearing it is the table's business (phase 0)."""

    def __init__(self, log2_entries, rows, max_discs=0):
        self.log2, self.rows, self.max_discs = log2_entries, rows, max_discs
        self.E, self.mask = 1 << log2_entries, (1 << log2_entries) - 1
        self.limit = max_discs or 64
        self.lay, self.bytes = sections(log2_entries, rows)
        self._raw = np.zeros(self.bytes + 256, dtype=np.uint8)
        o = (-self._raw.ctypes.data) % 256
        self.buf = self._raw[o:o + self.bytes]
        self.buf[:] = _rng(99).integers(0, 256, self.bytes, dtype=np.uint8)
        self._views()
        self.own, self.enemy = np.zeros(rows, dtype=np.uint64), np.zeros(rows, dtype=np.uint64)
        self.active = np.zeros(rows, dtype=np.uint8)
        self.policy, self.value = np.zeros((rows, 64), dtype=np.uint32), np.zeros(rows, dtype=np.uint32)

    def _views(self):
        for name, (off, n) in self.lay.items():
            setattr(self, name, self.buf[off:off + n].view(_DTYPES.get(name, np.uint32)))
        self.keys = self.keys.reshape(self.E, 2)
        self.pv = self.pv.reshape(self.E, 72)

    ARRAYS = ("buf", "own", "enemy", "active", "policy", "value")

    def copy(self):
        c = object.__new__(Rig)
        c.__dict__.update({k: v for k, v in self.__dict__.items() if k not in self.lay})
        for name in self.ARRAYS:
            setattr(c, name, getattr(self, name).copy())
        c._raw = None
        c._views()
        return c

    def same_bytes(self, other):
        return all(np.array_equal(getattr(self, n), getattr(other, n)) for n in self.ARRAYS)

    def place(self, own, enemy, active=1):
        """Rows 0 .. len - 1 hold the given positions; the other rows keep theirs."""
        own, enemy = _u(own), _u(enemy)
        assert not (own & enemy).any(), "not a position: a square of both colours"
        self.own[:len(own)], self.enemy[:len(own)] = own, enemy
        self.active[:] = 0
        self.active[:len(own)] = active


def call_args(rig, ptr, call, ov):
    """The arguments of raz_leaf_cache_probe (without the stream) for one call; ptr: {cache, own, enemy, active, policy, value} addresses.
    ov (the refusal tests): log2 / bytes / rows replace the rig's, null = names passed as NULL, shift = {name: bytes added}."""
    phase, p0, pn, part, step = call
    p = dict(ptr)
    for name in ov.get("null", ()):
        p[name] = None
    for name, d in ov.get("shift", {}).items():
        p[name] += d
    return (phase, p["cache"], ov.get("bytes", rig.bytes), ov.get("log2", rig.log2), rig.max_discs, ov.get("rows", rig.rows),
            p["own"], p["enemy"], p["active"], p["policy"], p["value"], p0, pn, part, step)


def ok(rcs):
    assert all(rc == 0 for rc in rcs), rcs


# ---------------------------------------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def pool():
    """200 000 seeded sparse positions (about 8 + 7 discs) with their tags: all distinct, and every home slot of a 2^10 table has at
    least 12 of them (it has some 150)."""
    r, n = _rng(2), 200000
    b = r.integers(0, 1 << 64, (6, n), dtype=np.uint64)
    own = b[0] & b[1] & b[2]
    enemy = b[3] & b[4] & b[5] & ~own
    tag = leaf_tag(own, enemy)
    assert len(np.unique(tag)) == n and not (own & enemy).any()
    assert np.bincount(home_slot(tag, 10), minlength=1024).min() >= 12
    return own, enemy, tag


def at_home(home, n, log2=10, skip=0):
    """n distinct positions (with distinct tags) whose home slot in a table of 2^log2 entries is `home`."""
    own, enemy, tag = pool()
    idx = np.flatnonzero(home_slot(tag, log2) == home)[skip:skip + n]
    assert len(idx) == n, f"only {len(idx)} positions at home slot {home}"
    return own[idx], enemy[idx]


def distinct_homes(n, log2=10, seed=3):
    """n positions with n different home slots: whatever the order of execution, each claims its home slot - room is guaranteed."""
    own, enemy, tag = pool()
    _, first = np.unique(home_slot(tag, log2), return_index=True)
    assert len(first) >= n
    idx = _rng(seed).permutation(first)[:n]
    assert len(np.unique(home_slot(tag[idx], log2))) == n
    return own[idx], enemy[idx]


@functools.lru_cache(maxsize=None)
def collisions(n=8):
    """n pairs (A, B) of different positions with the same tag: A from the pool; B from the other 64-bit value that `| 1` maps to A's
    tag, taken back through the finalizer, with an enemy of 4 discs chosen and own solved for (K1 is odd)."""
    own, enemy, _ = pool()
    r, out, draws, i = _rng(4), [], 0, 0
    while len(out) < n:
        a_own, a_enemy = int(own[i]), int(enemy[i])
        x0 = _unfin_int(int(pre_tag(a_own, a_enemy)[0]) ^ 1)
        assert _fin_int(x0) == int(pre_tag(a_own, a_enemy)[0]) ^ 1
        for _ in range(64):
            draws += 1
            e = sum(1 << int(s) for s in r.choice(64, 4, replace=False))
            o = ((x0 ^ (((e + K2) & MASK64) * K3 & MASK64)) * pow(K1, -1, 1 << 64)) & MASK64
            if o & e == 0:
                out.append((a_own, a_enemy, o, e))
                break
        i += 1
    assert draws < 4000
    a = np.array(out, dtype=np.uint64)
    A, B = (a[:, 0], a[:, 1]), (a[:, 2], a[:, 3])
    assert (leaf_tag(*A) == leaf_tag(*B)).all() and ((A[0] != B[0]) | (A[1] != B[1])).all()
    assert len(np.unique(home_slot(leaf_tag(*A), 10))) == n        # the pairs do not meet each other
    return A, B


def with_discs(k, n, seed):
    """n positions of exactly k discs."""
    r = _rng(1000 + 100 * seed + k)
    own, enemy = [], []
    for _ in range(n):
        sq = r.permutation(64)[:k]
        m = int(r.integers(0, k + 1))
        own.append(sum(1 << int(s) for s in sq[:m]))
        enemy.append(sum(1 << int(s) for s in sq[m:]))
    own, enemy = _u(own), _u(enemy)
    assert (discs_of(own, enemy) == k).all() and not (own & enemy).any()
    assert len(np.unique(leaf_tag(own, enemy))) == n
    return own, enemy


# ---------------------------------------------------------------------------------------------------------------- assertions
def _key(o, e):
    return (int(o), int(e))


def _eq(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: {a.tolist()[:12]} != {b.tolist()[:12]}"
    assert np.array_equal(a, b), f"{what}: differs at {np.argwhere(a != b)[:4].tolist()}"


class Seen:
    """What a `before` did, read from the arrays: per row its kind and entry."""

    def __init__(self, s0, s, p0, pn):
        rows = s.rows
        self.inside = np.zeros(rows, dtype=bool)
        self.inside[p0:p0 + pn] = True
        self.active0 = (s0.active != 0) & self.inside
        self.kind, self.entry = (s.role & 7).astype(np.int64), (s.role >> 3).astype(np.int64)
        self.tag = leaf_tag(s0.own, s0.enemy)
        self.home = home_slot(self.tag, s.log2)
        self.cacheable = discs_of(s0.own, s0.enemy) <= s.limit
        self.hit = self.active0 & (self.kind == NONE)

    def kinds(self, rows):
        return [("HIT" if self.hit[r] else ("NONE", "PLAIN", "OWN", "FOLLOW", "WAIT")[self.kind[r]]) for r in rows]


def check_before(s0, s, p0, pn, part, step, room=True):
    """s0: the arrays before the call, s: after it (or after the `after` that followed with no host work in between: nothing below
    is changed by a fill).  room: every position that is new to the table is guaranteed an entry by construction."""
    v = Seen(s0, s, p0, pn)
    rows, out = s.rows, ~v.inside
    _eq(s.own, s0.own, "own")
    _eq(s.enemy, s0.enemy, "enemy")
    for name in ("role", "active", "policy", "value"):                       # outside the slice: untouched
        _eq(getattr(s, name)[out], getattr(s0, name)[out], f"{name} outside the slice")
    idle = v.inside & ~v.active0                                              # inactive on entry: role NONE, still inactive, untouched
    assert (s.role[idle] == NONE).all() and (s.active[idle] == 0).all()
    _eq(s.policy[idle], s0.policy[idle], "policy of an inactive row")
    _eq(s.value[idle], s0.value[idle], "value of an inactive row")
    assert np.isin(v.kind[v.inside], (NONE, PLAIN, OWN, WAIT)).all(), "a FOLLOW role was left unresolved"
    # the compact list
    n = int(s.n_compact[part])
    lst = s.list[p0:p0 + n].astype(np.int64)
    assert n <= pn and len(np.unique(lst)) == n and (lst < pn).all(), ("compact list", n, lst[:8])
    listed = np.zeros(rows, dtype=bool)
    listed[p0 + lst] = True
    _eq(listed, v.active0 & np.isin(v.kind, (OWN, PLAIN)), "the listed rows are the OWN and PLAIN rows")
    _eq(s.active[v.inside], s0.active[v.inside] * listed[v.inside], "exactly the listed rows are still active")
    others = np.arange(16) != part
    _eq(s.n_compact[others], s0.n_compact[others], "another slice's count")
    # the table only grows, and only through claims
    used0 = s0.tags != 0
    for name in ("tags", "keys", "stamp", "owner"):
        _eq(getattr(s, name)[used0], getattr(s0, name)[used0], f"{name} of an entry that was taken")
    rdy0 = used0 & (s0.ready == 1)
    assert np.isin(s.ready, (0, 1)).all() and (s.ready[rdy0] == 1).all()
    _eq(s.pv[rdy0], s0.pv[rdy0], "pv of a ready entry")
    ready_of = {_key(*s0.keys[j]): j for j in np.flatnonzero(rdy0)}
    assert len(ready_of) == int(rdy0.sum()), "two ready entries hold one position"
    taken_tags0 = set(s0.tags[used0].tolist())
    claimed = []
    for r in np.flatnonzero(v.active0):
        key, k, i = _key(s0.own[r], s0.enemy[r]), v.kind[r], v.entry[r]
        if not v.cacheable[r]:
            assert k == PLAIN, f"row {r}: {int(discs_of(*key)[0])} discs > {s.limit} must be PLAIN, is {v.kinds([r])}"
            continue
        if key in ready_of:
            assert v.hit[r], f"row {r}: its position is ready in entry {ready_of[key]} but the row is {v.kinds([r])}"
        if v.hit[r]:
            assert key in ready_of, f"row {r} was served as a hit, but no ready entry holds its position"
            j = ready_of[key]
            assert s0.tags[j] == v.tag[r] and ((j - v.home[r]) & s.mask) < PROBES
            assert np.array_equal(s.policy[r], s0.pv[j, :64]) and s.value[r] == s0.pv[j, 64], f"hit row {r}: not the bits of entry {j}"
            assert s.active[r] == 0 and s.role[r] == NONE
        elif k == WAIT:
            assert _key(*s.keys[i]) == key and s.tags[i] == v.tag[r], f"row {r} waits for entry {i}, which holds another position"
            assert s.stamp[i] == step, f"row {r} waits for entry {i} claimed in step {s.stamp[i]}, not {step}"
            ow = int(s.owner[i])
            assert p0 <= ow < p0 + pn and ow != r, f"row {r} waits for row {ow}, outside its slice [{p0}, {p0 + pn})"
            assert s.role[ow] == ((i << 3) | OWN), f"row {r} waits for row {ow}, which does not own entry {i}"
            assert s.active[r] == 0
        elif k == OWN:
            assert not used0[i] and s.tags[i] == v.tag[r] and _key(*s.keys[i]) == key, f"row {r} owns entry {i}: tag / key"
            assert s.stamp[i] == step and s.owner[i] == r and ((i - v.home[r]) & s.mask) < PROBES, f"row {r} owns entry {i}: stamp / owner / window"
            claimed.append(i)
        else:
            assert k == PLAIN
    assert len(set(claimed)) == len(claimed), "two rows own one entry"
    _eq(np.flatnonzero(~used0 & (s.tags != 0)), np.array(sorted(claimed), dtype=np.int64), "the new entries are the owned ones")
    # a position new to the table, alone with its tag: one row owns it, the others wait
    if room:
        groups, tags_in_batch = {}, {}
        for r in np.flatnonzero(v.active0 & v.cacheable):
            key = _key(s0.own[r], s0.enemy[r])
            groups.setdefault(key, []).append(r)
            tags_in_batch.setdefault(int(v.tag[r]), set()).add(key)
        for key, rs in groups.items():
            t = int(v.tag[rs[0]])
            if t in taken_tags0 or len(tags_in_batch[t]) > 1:
                continue
            ks = sorted(v.kind[rs].tolist())
            assert ks == [OWN] + [WAIT] * (len(rs) - 1), f"rows {rs[:6]} of one new position: {v.kinds(rs[:6])}"
    # counters
    d = s.counters.astype(np.int64) - s0.counters.astype(np.int64)
    window = s.tags[(v.home[:, None] + np.arange(PROBES)[None, :]) & s.mask]
    no_room = v.active0 & v.cacheable & (v.kind == PLAIN) & ~(window == v.tag[:, None]).any(axis=1)
    assert (window[no_room] != 0).all()
    want = [int(v.hit.sum()), int((v.active0 & (v.kind == WAIT)).sum()), n, int(no_room.sum()), 0, 0, 0, 0]
    assert d.tolist() == want, f"counter deltas {d.tolist()}, want {want}"
    assert d[0] + d[1] + d[2] == int(v.active0.sum())
    return v


def check_ready_entries(s):
    """Every entry with ready == 1 holds net(its key) in pv[0 .. 65); words 65 .. 71 are padding."""
    rdy = np.flatnonzero(s.ready == 1)
    assert np.isin(s.ready, (0, 1)).all() and (s.tags[rdy] != 0).all()
    assert (s.tags[rdy] == leaf_tag(s.keys[rdy, 0], s.keys[rdy, 1])).all()
    want = net(s.keys[rdy, 0], s.keys[rdy, 1])
    bad = np.flatnonzero((s.pv[rdy, :65] != want).any(axis=1))
    assert len(bad) == 0, f"{len(bad)} ready entries do not hold the answer of their key, first entry {rdy[bad[0]]}"
    return rdy


def check_after(s0, s1, s, v, p0, pn, part, step, fill_step):
    """s0: before the `before`; s1: just before the `after` (None where both ran back to back); s: now."""
    want = net(s0.own, s0.enemy)
    a = v.active0
    bad = np.flatnonzero(a & ((s.policy != want[:, :64]).any(axis=1) | (s.value != want[:, 64])))
    assert len(bad) == 0, f"rows {bad[:8].tolist()} ({v.kinds(bad[:8])}) do not hold the answer of their position"
    ref = s1 if s1 is not None else s0
    _eq(s.policy[~a], ref.policy[~a], "policy of a row that was not active")
    _eq(s.value[~a], ref.value[~a], "value of a row that was not active")
    if s1 is not None:
        for name in ("role", "active", "list", "n_compact", "counters", "tags", "keys", "stamp", "owner"):
            _eq(getattr(s, name), getattr(s1, name), f"{name} across the fill")
    if s1 is None:                                                            # (otherwise the `before` checked them, and the fill left them alone)
        d = s.counters.astype(np.int64) - s0.counters.astype(np.int64)
        assert d[2] == int(s.n_compact[part]) and d[0] + d[1] + d[2] == int(a.sum())
    check_ready_entries(s)
    owned = np.sort(v.entry[a & (v.kind == OWN)]) if fill_step == step else np.zeros(0, dtype=np.int64)
    _eq(np.flatnonzero((s.ready == 1) & ~((ref.ready == 1) & (ref.tags != 0))), owned, "the entries that became ready are this step's owned ones")


class Ctx:
    pass


def before(run, rig, p0, pn, part, step, room=True):
    """Poison mode, first half: policy and value of every row poisoned, `before`, assertions, then the host plays the net for exactly
    the listed rows."""
    c = Ctx()
    c.args = (p0, pn, part, step)
    rig.policy[:], rig.value[:] = POISON, POISON
    c.s0 = rig.copy()
    ok(run(rig, [(BEFORE, p0, pn, part, step)]))
    c.v = check_before(c.s0, rig, p0, pn, part, step, room)
    return c


def host_net(rig, c):
    p0, pn, part, _ = c.args
    rows = p0 + rig.list[p0:p0 + int(rig.n_compact[part])].astype(np.int64)
    w = net(rig.own[rows], rig.enemy[rows])
    rig.policy[rows], rig.value[rows] = w[:, :64], w[:, 64]


def after(run, rig, c, fill_step=None):
    p0, pn, part, step = c.args
    fill_step = step if fill_step is None else fill_step
    s1 = rig.copy()
    ok(run(rig, [(AFTER, p0, pn, part, fill_step)]))
    check_after(c.s0, s1, rig, c.v, p0, pn, part, step, fill_step)
    return c.v


def one_step(run, rig, p0, pn, part, step, mode="poison", room=True):
    """One slice, one step, in either mode; returns what the rows did (Seen)."""
    if mode == "poison":
        c = before(run, rig, p0, pn, part, step, room)
        host_net(rig, c)
        return after(run, rig, c)
    w = net(rig.own, rig.enemy)                                               # prefilled: every row holds its answer, the phases run back to back
    rig.policy[:], rig.value[:] = w[:, :64], w[:, 64]
    s0 = rig.copy()
    ok(run(rig, [(BEFORE, p0, pn, part, step), (AFTER, p0, pn, part, step)]))
    v = check_before(s0, rig, p0, pn, part, step, room)
    check_after(s0, None, rig, v, p0, pn, part, step, step)
    return v


def fresh(run, log2, rows, max_discs=0):
    rig = Rig(log2, rows, max_discs)
    ok(run(rig, [(CLEAR, 0, 0, 0, 0)]))
    for name in ("tags", "stamp", "ready", "counters", "n_compact", "role"):
        assert not getattr(rig, name).any(), name
    return rig


# ---------------------------------------------------------------------------------------------------------------- scenarios
def case_hash_and_layout(run):
    """One active row in a cleared table: exactly one tag, at the restated home slot, equal to the restated tag; key, stamp, owner as
    given; ready after the fill.  This pins the restatements above against the kernel."""
    (ao, ae), (bo, be) = collisions()
    f63, f64 = with_discs(63, 1, 0), with_discs(64, 1, 0)
    po, pe = distinct_homes(4, 11, seed=5)
    own = np.concatenate([_u([INIT_OWN, 0, 1 << 63]), ao[:2], bo[:2], f63[0], f64[0], po])
    enemy = np.concatenate([_u([INIT_ENEMY, 1, 0]), ae[:2], be[:2], f63[1], f64[1], pe])
    for n, (o, e) in enumerate(zip(own, enemy)):
        for log2 in (10, 11):
            rig = fresh(run, log2, 7)
            r, step = n % 7, 1 + n
            rig.own[r], rig.enemy[r], rig.active[r] = o, e, 1
            v = one_step(run, rig, 0, 7, n % 16, step, MODES[n % 2])
            tag = int(leaf_tag(o, e)[0])
            h = (tag >> 24) & rig.mask
            assert np.flatnonzero(rig.tags).tolist() == [h] and int(rig.tags[h]) == tag and tag & 1
            assert _key(*rig.keys[h]) == _key(o, e) and rig.stamp[h] == step and rig.owner[h] == r and rig.ready[h] == 1
            assert rig.role[r] == ((h << 3) | OWN) and v.kinds([r]) == ["OWN"]
            assert rig.list[0] == r and rig.n_compact[n % 16] == 1 and rig.counters.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]


def case_collision_a_ready_b_arrives(run, rig=None):
    """A is ready in the table; B (same tag, another key) arrives together with A: A is a hit, B is evaluated, is not a hit and is not
    stored.  Returns the rig and what a later run of the same calls must reproduce (no two rows of a batch compete here)."""
    (ao, ae), (bo, be) = collisions()
    n = len(ao)
    assert n >= 8
    rig = rig or fresh(run, 10, 2 * n + 3)
    trace = []
    steps = [("poison", (ao, ae), ["OWN"] * n),
             ("poison", (np.concatenate([bo, ao]), np.concatenate([be, ae])), ["PLAIN"] * n + ["HIT"] * n),
             ("prefilled", (np.concatenate([ao, bo]), np.concatenate([ae, be])), ["HIT"] * n + ["PLAIN"] * n)]   # and with the streams running free
    for t, (mode, (o, e), want) in enumerate(steps):
        rig.place(o, e)
        taken = np.flatnonzero(rig.tags)
        v = one_step(run, rig, 0, len(o), t, 1 + t, mode)
        assert v.kinds(range(len(o))) == want, (t, v.kinds(range(len(o))))
        if t:
            _eq(np.flatnonzero(rig.tags), taken, "B must not be stored")
        trace.append((rig.role.copy(), rig.counters.copy(), rig.policy.copy(), rig.value.copy(), rig.tags.copy(), rig.ready.copy()))
    assert rig.counters.tolist()[:4] == [2 * n, 0, 3 * n, 0]
    return rig, trace


def case_collision_same_batch(run):
    """A and B in one batch, empty table: whichever claims the entry owns it; the other matches the tag, fails the key comparison and
    is evaluated.  Neither may wait for the other."""
    (ao, ae), (bo, be) = collisions()
    n = len(ao)
    for mode in MODES:
        for order in (0, 1):
            rig = fresh(run, 10, 4 * n)
            o = np.concatenate([ao, bo, ao, bo] if order == 0 else [bo, ao, bo, ao])
            e = np.concatenate([ae, be, ae, be] if order == 0 else [be, ae, be, ae])
            rig.place(o, e)
            v = one_step(run, rig, 0, 4 * n, 3, 9, mode, room=False)
            for i in range(n):
                rs = [i, n + i, 2 * n + i, 3 * n + i]
                ks = sorted(v.kinds(rs))
                assert ks == ["OWN", "PLAIN", "PLAIN", "WAIT"], (i, v.kinds(rs))   # the owner's twin waits, both rows of the other position are evaluated
            assert int((rig.tags != 0).sum()) == n and int(rig.counters[3]) == 0
            rig.active[:] = 1
            v = one_step(run, rig, 0, 4 * n, 3, 10, mode, room=False)               # next step: the stored ones are hits, the others evaluated again
            assert sorted(v.kinds(range(4 * n))) == ["HIT"] * (2 * n) + ["PLAIN"] * (2 * n)


def case_collision_a_unfinished(run):
    """B arrives while A is claimed but not filled - in a later step of the same slice, and in the same step from another slice."""
    (ao, ae), (bo, be) = collisions()
    n = len(ao)
    for later in (True, False):
        rig = fresh(run, 10, 2 * n)
        rig.place(np.concatenate([ao, bo]), np.concatenate([ae, be]))
        c0 = before(run, rig, 0, n, 0, 3)
        assert c0.v.kinds(range(n)) == ["OWN"] * n
        rig.active[:] = 1
        if later:
            c1 = before(run, rig, n, n, 0, 4)
        else:
            c1 = before(run, rig, n, n, 1, 3)
        assert c1.v.kinds(range(n, 2 * n)) == ["PLAIN"] * n
        host_net(rig, c1)
        after(run, rig, c1)
        assert not rig.ready.any() and int((rig.tags != 0).sum()) == n


def _groups_run(run, groups, mode, seed):
    """groups: [(home, n)] in a table of 2^10 entries, home slots at least 16 apart: n distinct positions at each home."""
    homes = sorted(h for h, _ in groups)
    assert all((b - a) >= 16 for a, b in zip(homes, homes[1:])) and (len(homes) < 2 or homes[0] + 1024 - homes[-1] >= 16)
    own = np.concatenate([at_home(h, n)[0] for h, n in groups])
    enemy = np.concatenate([at_home(h, n)[1] for h, n in groups])
    grp = np.concatenate([np.full(n, g) for g, (_, n) in enumerate(groups)])
    perm = _rng(seed).permutation(len(own))
    own, enemy, grp = own[perm], enemy[perm], grp[perm]
    rig = fresh(run, 10, len(own) + 2)
    rig.place(own, enemy)
    v = one_step(run, rig, 0, len(own), 5, 21, mode, room=False)
    want_entries, lost = [], 0
    for g, (h, n) in enumerate(groups):
        rs = np.flatnonzero(grp == g)
        ks = v.kinds(rs)
        assert ks.count("OWN") == min(PROBES, n) and ks.count("PLAIN") == n - min(PROBES, n), (h, n, ks)
        want_entries += [(h + k) & 1023 for k in range(min(PROBES, n))]
        lost += n - min(PROBES, n)
    assert np.flatnonzero(rig.tags).tolist() == sorted(want_entries), (groups, np.flatnonzero(rig.tags).tolist())
    assert rig.counters.tolist()[:4] == [0, 0, len(own), lost]
    rig.active[:len(own)] = 1                                                  # next step: the stored are hits, the rest find no room again
    v2 = one_step(run, rig, 0, len(own), 5, 22, mode, room=False)
    assert [k == "HIT" for k in v2.kinds(range(len(own)))] == [k == "OWN" for k in v.kinds(range(len(own)))]
    assert rig.counters.tolist()[:4] == [len(own) - lost, 0, len(own) + lost, 2 * lost]


def case_same_home_slot(run):
    """8, 9 and 12 positions at one home slot: min(8, n) claims, the rest find no room; the exact entries taken."""
    for i, mode in enumerate(MODES):
        _groups_run(run, [(100, 8), (300, 9), (501, 12), (0, 3), (40, 1)], mode, 10 + i)


def case_window_wraps(run):
    """The same at home slots mask, mask - 3 and mask - 7: the window continues at entries 0 .. 6."""
    i = 0
    for h in (1023, 1020, 1016):
        for n in (8, 9, 12):
            _groups_run(run, [(h, n), (500, (8, 9, 12)[(i + 1) % 3])], MODES[i % 2], 20 + i)
            i += 1


def case_max_discs(run):
    """11, 12, 13 discs at max_discs = 12; 63, 64 discs at max_discs = 0 (= 64) and 64."""
    for mode in MODES:
        for max_discs, ks, shallow in ((12, (11, 12, 13), (11, 12)), (0, (63, 64), (63, 64)), (64, (63, 64), (63, 64)), (63, (63, 64), (63,))):
            per = 5
            pos = [with_discs(k, per, max_discs) for k in ks]
            own = np.concatenate([p[0] for p in pos] * 2)                      # every position twice
            enemy = np.concatenate([p[1] for p in pos] * 2)
            k_of = np.concatenate([np.full(per, k) for k in ks] * 2)
            rig = fresh(run, 10, len(own), max_discs)
            assert len(np.unique(home_slot(leaf_tag(own, enemy), 10))) == len(own) // 2   # room for every one
            rig.place(own, enemy)
            v = one_step(run, rig, 0, len(own), 0, 1, mode)
            for k in ks:
                got = sorted(v.kinds(np.flatnonzero(k_of == k)))
                assert got == (["OWN"] * per + ["WAIT"] * per if k in shallow else ["PLAIN"] * 2 * per), (max_discs, k, got)
            assert int(rig.counters[3]) == 0 and int((rig.tags != 0).sum()) == per * len(shallow)
            rig.active[:] = 1
            v = one_step(run, rig, 0, len(own), 0, 2, mode)
            for k in ks:
                assert set(v.kinds(np.flatnonzero(k_of == k))) == ({"HIT"} if k in shallow else {"PLAIN"}), (max_discs, k)


PNS, P0S, PARTS = (1, 3, 4, 5, 255, 256, 257), (0, 5, 256), (0, 1, 15)


def case_slice_shapes(run, content, pns=PNS, p0s=P0S, parts=PARTS):
    """pn around the claim kernel's 256-row block and the 4 rows per block of resolve and fill, p0 = 0 / odd / a block further, every
    `part`; 600 rows, the rows around the slice active and poisoned.  content: 'distinct' - every row another position; 'same' - one
    position in every row (one OWN, pn - 1 WAIT); 'mix' - pairs of rows share a position, every third row inactive.  Then the same
    slice again at step + 1, the phases back to back: every cacheable row is a hit, nothing is listed."""
    po, pe = distinct_homes(600, 10, seed=6)
    n = 0
    for pn in pns:
        for p0 in p0s:
            for part in parts:
                n += 1
                rig = fresh(run, 10, 600)
                j = np.arange(600)
                idx = {"distinct": j, "same": np.full(600, 17 + n), "mix": j // 2}[content]
                rig.place(po[idx], pe[idx])
                if content == "mix":
                    rig.active[j % 3 == 2] = 0
                a0 = rig.active.copy()
                rig.n_compact[:] = 77                                          # (the claim resets its slice's count, and that one alone)
                v = one_step(run, rig, p0, pn, part, 2 * n + 1, "poison")
                inside = a0[p0:p0 + pn] != 0
                ks = v.kinds(np.arange(p0, p0 + pn)[inside])
                if content == "distinct":
                    assert ks == ["OWN"] * pn
                elif content == "same":
                    assert sorted(ks) == ["OWN"] + ["WAIT"] * (pn - 1)
                else:
                    assert ks.count("OWN") == len(set(idx[p0:p0 + pn][inside])) and ks.count("WAIT") == len(ks) - ks.count("OWN")
                assert rig.n_compact[part] == ks.count("OWN") and (np.delete(rig.n_compact, part) == 77).all()
                rig.active[:] = a0
                v = one_step(run, rig, p0, pn, part, 2 * n + 2, "prefilled")
                assert set(v.kinds(np.arange(p0, p0 + pn)[inside])) <= {"HIT"} and rig.n_compact[part] == 0
                _eq(rig.active[p0:p0 + pn], np.zeros(pn, dtype=np.uint8), "every row of the slice was served")
    assert n == len(pns) * len(p0s) * len(parts)


def case_stale_owner(run):
    """A claim whose step never finished: its entry is never followed and never filled - the rows asking for it are evaluated, in
    every later step."""
    po, pe = distinct_homes(6, 10, seed=7)
    rig = fresh(run, 10, 8)
    rig.place(po[:4], pe[:4])
    c = before(run, rig, 0, 4, 0, 7)
    assert c.v.kinds(range(4)) == ["OWN"] * 4
    dead = int(c.v.entry[0])
    for step, mode in ((8, "poison"), (9, "prefilled"), (10, "poison")):
        rig.place(np.array([po[4], po[5], po[0], po[0]]), np.array([pe[4], pe[5], pe[0], pe[0]]))
        if mode == "poison":
            c = before(run, rig, 0, 4, 0, step)
            assert c.v.kinds(range(4)) == (["OWN", "OWN"] if step == 8 else ["HIT", "HIT"]) + ["PLAIN", "PLAIN"]
            assert sorted(rig.list[:int(rig.n_compact[0])].tolist())[-2:] == [2, 3]
            host_net(rig, c)
            after(run, rig, c)
        else:
            v = one_step(run, rig, 0, 4, 0, step, mode)
            assert v.kinds(range(4)) == ["HIT", "HIT", "PLAIN", "PLAIN"]
        assert rig.ready[dead] == 0 and rig.stamp[dead] == 7 and rig.owner[dead] == 0
    assert int(rig.ready.sum()) == 2 and int(rig.counters[3]) == 0


def case_wrong_step_fill(run):
    """`before` at step 5, `after` at step 6: no entry becomes ready, and waiting rows still receive their owner's answer."""
    po, pe = distinct_homes(3, 10, seed=8)
    idx = [0, 0, 1, 1, 2, 0, 1]
    rig = fresh(run, 10, 9)
    rig.place(po[idx], pe[idx])
    rig.active[7:] = 1                                                         # (rows beyond the slice: active, poisoned, untouched)
    c = before(run, rig, 0, 7, 2, 5)
    assert sorted(c.v.kinds(range(7))) == ["OWN"] * 3 + ["WAIT"] * 4
    host_net(rig, c)
    after(run, rig, c, fill_step=6)
    assert not rig.ready.any()
    rig.active[:7] = 1
    v = one_step(run, rig, 0, 7, 2, 6, "poison")                              # dead weight, not a wrong answer: all are evaluated from now on
    assert v.kinds(range(7)) == ["PLAIN"] * 7 and not rig.ready.any()


def case_owner_in_another_slice(run):
    """The same positions in rows [0, 8) and [8, 16), same step value: the second slice's rows find the first slice's claims and must
    not wait for them - they are evaluated."""
    po, pe = distinct_homes(8, 10, seed=9)
    rig = fresh(run, 10, 16)
    rig.place(np.concatenate([po, po]), np.concatenate([pe, pe]))
    c0 = before(run, rig, 0, 8, 0, 3)
    c1 = before(run, rig, 8, 8, 1, 3)
    assert c0.v.kinds(range(8)) == ["OWN"] * 8 and c1.v.kinds(range(8, 16)) == ["PLAIN"] * 8
    host_net(rig, c0)
    host_net(rig, c1)
    after(run, rig, c0)
    after(run, rig, c1)
    assert int(rig.ready.sum()) == 8 and rig.counters.tolist()[:4] == [0, 0, 16, 0]


def case_reattach(run):
    """A used table, cleared: roles, counters and answers of the first scenario are those of a fresh buffer; the keys, owners and
    answers the first use left behind change nothing."""
    rig, first = case_collision_a_ready_b_arrives(run)
    stale = rig.copy()
    assert stale.tags.any() and stale.ready.any() and stale.counters.any() and stale.role.any()
    ok(run(rig, [(CLEAR, 0, 0, 0, 0)]))
    for name in ("tags", "stamp", "ready", "counters", "n_compact", "role"):
        assert not getattr(rig, name).any(), name
    for name in ("keys", "owner", "pv"):
        _eq(getattr(rig, name), getattr(stale, name), name)
    _, second = case_collision_a_ready_b_arrives(run, rig)
    for a, b in zip(first, second):
        for x, y in zip(a, b):
            _eq(x, y, "after the clear")


def case_refusals(run):
    """Every refused call returns RAZ_EINVAL and leaves every buffer byte for byte as it was."""
    po, pe = distinct_homes(8, 10, seed=11)
    rig = fresh(run, 10, 8)
    rig.place(po, pe)
    one_step(run, rig, 0, 8, 0, 1, "poison")
    rig.active[:] = 1
    snap = rig.copy()
    good = (BEFORE, 0, 8, 0, 2)
    refused = [((3, 0, 8, 0, 2), {}), ((-1, 0, 8, 0, 2), {}), (good, {"log2": 9}), (good, {"log2": 29}), (good, {"bytes": rig.bytes - 1}),
               (good, {"bytes": 0}), (good, {"null": ("cache",)}), (good, {"shift": {"cache": 8}}), (good, {"shift": {"cache": 128}}),
               (good, {"shift": {"own": 4}}), (good, {"shift": {"enemy": 4}}), (good, {"shift": {"policy": 2}}), (good, {"shift": {"value": 1}}),
               ((BEFORE, 1, 8, 0, 2), {}), ((BEFORE, 8, 1, 0, 2), {}), ((AFTER, 0, 9, 0, 2), {}), ((CLEAR, 0, 9, 0, 0), {}),
               ((BEFORE, 0xffffffff, 2, 0, 2), {}), ((BEFORE, 0, 8, 16, 2), {}), ((AFTER, 0, 8, 0xffffffff, 2), {}),
               ((BEFORE, 0, 0, 0, 2), {}), ((AFTER, 0, 0, 0, 2), {}), ((BEFORE, 8, 0, 0, 2), {})]
    refused += [(good, {"null": (name,)}) for name in ("own", "enemy", "active", "policy", "value")]
    refused += [((CLEAR, 0, 0, 0, 0), {"null": ("cache",)}), ((CLEAR, 0, 0, 0, 0), {"log2": 11})]   # (a 2^11 table does not fit this buffer)
    for call, ov in refused:
        assert run(rig, [call], **ov) == [RAZ_EINVAL], (call, ov)
        assert rig.same_bytes(snap), (call, ov)
    v = one_step(run, rig, 0, 8, 0, 2, "poison")                              # and the accepted form of the same call works
    assert v.kinds(range(8)) == ["HIT"] * 8


CASES = {
    "hash_and_layout": case_hash_and_layout,
    "collision_a_ready_b_arrives": lambda run: case_collision_a_ready_b_arrives(run) and None,
    "collision_same_batch": case_collision_same_batch,
    "collision_a_unfinished": case_collision_a_unfinished,
    "same_home_slot": case_same_home_slot,
    "window_wraps": case_window_wraps,
    "max_discs": case_max_discs,
    "slices_distinct": lambda run: case_slice_shapes(run, "distinct"),
    "slices_same": lambda run: case_slice_shapes(run, "same"),
    "slices_mix": lambda run: case_slice_shapes(run, "mix"),
    "stale_owner": case_stale_owner,
    "wrong_step_fill": case_wrong_step_fill,
    "owner_in_another_slice": case_owner_in_another_slice,
    "reattach": case_reattach,
    "refusals": case_refusals,
}
