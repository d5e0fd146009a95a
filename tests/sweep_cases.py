"""Inputs, references and assertions for the seven batched sweep entries of csrc/raz_sweep.hip (include/raz.h raz_*_batch) with their
LOOPS taking several trips.  Shared by tests/test_sweep_loops_gpu.py (the device, through lib/bitboard.py's wrappers) and
tests/test_sweep_loops_emu.py (the wave emulator, through the C ABI on host arrays): a case takes a DRIVER and knows nothing of where
the kernels execute.  Every comparison is exact.

The driver (numpy arrays in, numpy arrays out; `offsets` = {argument name: bytes} places that argument so many bytes behind a 256-byte
boundary; a refused call raises Refused with the outputs as the call left them):
    legal_moves(own, enemy)                       -> legal
    calc_flip(pos, own, enemy)                    -> flipped
    step(black, white, player, status, action)    -> black, white, player, status, legal      (the entry works in place on copies)
    score(black, white)                           -> winner, diff
    d4(x, sym)                                    -> out
    planes(own, enemy)                            -> float32 [n, 128]
    pick_kth(legal, rnd)                          -> action
    forms(n) -> (legal_moves_form, step_form)     raz_sweep_forms
    max_grid() -> workgroups                      raz_sweep_max_grid
    allocates                                     the output names the driver cannot place itself (the wrappers allocate them)

THE LAUNCH ARITHMETIC, restated (trips() below; G = max_grid(), 65536 unless RAZ_SWEEP_MAXGRID lowers it; a workgroup is 256 threads =
4 waves except on the sliced kernels, where it is one wave; grid_for(w) = min(max(ceil(w / 256), 1), G)):
  * raz_legal_moves_batch / raz_step_batch put nsb = n // 2048 whole superblocks on the sliced form forms(n) names (none on form 0)
    and the other r = n - 2048 nsb boards on k_legal_moves / k_step.
      - k_legal_moves_sliced, k_step_sliced, k_step_hybrid: min(nsb, G) waves (the hybrid also at most RAZ_SWEEP_HYBRID_WAVES, which
        these tests leave unset); wave w takes the superblocks w, w + grid, ...
      - k_legal_moves, k_step: grid_for(r // 4 + 1) workgroups; wave w of 4 grid takes the blocks w, w + 4 grid, ... of the r // 256
        whole blocks of 256 boards, loading block i + 4 grid before it computes and stores block i (the software pipeline); the
        r % 256 boards after them are the ragged tail, a board per thread.
  * k_calc_flip, k_score, k_d4: grid_for(n // 2 + 1) workgroups, a thread strides over the n // 2 pairs; an odd last board by thread 0.
  * k_pick_kth: grid_for(n) workgroups, a thread strides over the n boards.
  * k_planes: grid_for(64 n) workgroups, a WAVE strides over the n boards.
At G = 65536 a second trip needs 2^18 (k_planes) .. 2^27 (the sliced kernels) boards.  At G = 2 or 1, N_LOOP = 5 * 2048 + 307 boards
give every loop at least three: five superblocks (odd: two waves take 3 and 2), 41 blocks of 256 (8 waves: one takes 6, seven take 5)
and a ragged tail of 51 boards, an odd count.

ACTIONS 64..254.  The reference asserts 0 <= action <= 63 and the oracle's C port shifts by the action (undefined from 64 on), so
neither says what such a byte does; include/raz.h does: it names no square, flips nothing, and the mover loses (status | 0x10, the
board untouched) - step_reference applies exactly that to those boards and the oracle's step to all the others."""
import functools

import numpy as np

import oracle as O

RAZ_EINVAL = -1
DEFAULT_MAX_GRID = 65536
N_LOOP = 5 * 2048 + 307
EDGES = (0, 1, 2, 3, 255, 256, 257, 511, 513)
SIZES = EDGES + (N_LOOP,)
ENTRIES = ("legal_moves", "calc_flip", "step", "score", "d4", "planes", "pick_kth")
U = np.uint64
SENTINEL = 0xA5

# the configurations the test files run in children of their own (the library reads the variables once per process), and the
# kernels whose loops must take >= 3 trips on N_LOOP boards there (>= 2 on the least busy wave or thread that has any)
_STREAMING = ("k_calc_flip", "k_score", "k_d4", "k_planes", "k_pick_kth")
CONFIGS = {
    "a": dict(env={"RAZ_SWEEP_MAXGRID": "2"}, max_grid=2, forms=(0, 0), looped=("k_legal_moves", "k_step") + _STREAMING),
    "b": dict(env={"RAZ_SWEEP_MAXGRID": "1"}, max_grid=1, forms=(0, 0), looped=("k_legal_moves", "k_step") + _STREAMING),
    "c": dict(env={"RAZ_SWEEP_MAXGRID": "2", "RAZ_SWEEP_SLICED_MIN": "2048"}, max_grid=2, forms=(1, 2),
              looped=("k_legal_moves_sliced", "k_step_hybrid") + _STREAMING),
    "d": dict(env={"RAZ_SWEEP_MAXGRID": "2", "RAZ_SWEEP_SLICED_MIN": "2048", "RAZ_SWEEP_SLICED_STEP": "1"}, max_grid=2, forms=(1, 1),
              looped=("k_legal_moves_sliced", "k_step_sliced") + _STREAMING),
    "e": dict(env={"RAZ_SWEEP_MAXGRID": "1", "RAZ_SWEEP_SLICED_MIN": "2048"}, max_grid=1, forms=(1, 2),
              looped=("k_legal_moves_sliced", "k_step_hybrid") + _STREAMING),
}
KERNELS_OF = {"legal_moves": ("k_legal_moves", "k_legal_moves_sliced"), "step": ("k_step", "k_step_sliced", "k_step_hybrid"),
              "calc_flip": ("k_calc_flip",), "score": ("k_score",), "d4": ("k_d4",), "planes": ("k_planes",), "pick_kth": ("k_pick_kth",)}


class Refused(RuntimeError):
    """A call the entry refused: .rc (the emulator: the code returned; the device: None, the wrapper raised), .message, .outputs
    {name: array as the call left it}."""

    def __init__(self, rc, message, outputs):
        super().__init__(message)
        self.rc, self.message, self.outputs = rc, message, outputs


# ------------------------------------------------------------------------------------------------------------------ the launch arithmetic
def _share(items, workers):
    """(trips of the busiest worker, trips of the least busy worker that has any) when worker w takes the items w, w + workers, ..."""
    if items == 0:
        return 0, 0
    return -(-items // workers), max(items // workers, 1)


def _grid_for(work, G):
    return min(max(-(-work // 256), 1), G)


def trips(max_grid, forms, n):
    """{kernel: (busiest, least busy that has any)} - how often the loop of each kernel a batch of n boards launches goes round, on
    the wave (thread, for the pair / board striders) that takes most and on the one that takes least; (0, 0) = not launched or nothing
    to loop over.  RAZ_SWEEP_HYBRID_WAVES is taken as unset."""
    G, (lf, sf) = int(max_grid), forms
    nsb = n // 2048
    out = {}
    for name, form, lane_kernel, sliced in (("legal", lf, "k_legal_moves", {1: "k_legal_moves_sliced"}),
                                            ("step", sf, "k_step", {1: "k_step_sliced", 2: "k_step_hybrid"})):
        for k in sliced.values():
            out[k] = (0, 0)
        done = nsb if form else 0
        if done:
            out[sliced[form]] = _share(done, min(done, G))
        r = n - 2048 * done
        out[lane_kernel] = _share(r // 256, 4 * _grid_for(r // 4 + 1, G)) if r else (0, 0)
    for k in ("k_calc_flip", "k_score", "k_d4"):
        out[k] = _share(n // 2, 256 * _grid_for(n // 2 + 1, G)) if n else (0, 0)
    out["k_pick_kth"] = _share(n, 256 * _grid_for(n, G)) if n else (0, 0)
    out["k_planes"] = _share(n, 4 * _grid_for(64 * n, G)) if n else (0, 0)
    return out


def first_and_last_superblocks(max_grid, n):
    """The superblocks that are the FIRST and the LAST a wave of a sliced kernel takes."""
    nsb = n // 2048
    grid = min(nsb, int(max_grid))
    walks = [list(range(w, nsb, grid)) for w in range(grid)]
    return {w[0] for w in walks}, {w[-1] for w in walks}


# ------------------------------------------------------------------------------------------------------------------ bits
def bits_of(a):
    """uint8 [n, 64]: column s = bit s of a[i] (bit 0 = the top-left square)."""
    a = np.ascontiguousarray(a, dtype="<u8")
    return np.unpackbits(a.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little")


def words_of(bits):
    return np.packbits(np.ascontiguousarray(bits, dtype=np.uint8).reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1).astype(np.uint64)


def popcount(a):
    return bits_of(a).sum(axis=1).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------ restatements
def score_reference(black, white):
    """_game_over's count: winner 1 black / 2 white / 3 draw, diff = discs of black - discs of white as int8 (-64 .. 64)."""
    d = popcount(black) - popcount(white)
    return np.where(d > 0, 1, np.where(d < 0, 2, 3)).astype(np.uint8), d.astype(np.int8)


def planes_reference(own, enemy):
    return np.concatenate([bits_of(own), bits_of(enemy)], axis=1).astype(np.float32)


def pick_kth_reference(legal, rnd):
    """The k-th set bit (from bit 0) with k = rnd mod popcount, rnd UNSIGNED 32 bits; 255 for an empty mask."""
    b = bits_of(legal).astype(np.int64)
    pc = b.sum(axis=1)
    k = np.asarray(rnd, dtype=np.uint32).astype(np.int64) % np.maximum(pc, 1)
    hit = (b == 1) & (np.cumsum(b, axis=1) == (k + 1)[:, None])
    return np.where(pc == 0, 255, hit.argmax(axis=1)).astype(np.uint8)


def d4_reference(x, sym):
    """sym = 4 flip + rot: flip_vertical (row r <-> row 7 - r) first, then rot right rotations (rotate90 = flip_vertical, then the
    transposition that exchanges row and column)."""
    sym = np.asarray(sym, dtype=np.uint8)
    g = bits_of(x).reshape(-1, 8, 8)                      # [board, row, column]
    out = np.zeros_like(g)
    for s in range(8):
        h = g[:, ::-1, :] if s & 4 else g
        for _ in range(s & 3):
            h = h[:, ::-1, :].transpose(0, 2, 1)
        out[sym == s] = h[sym == s]
    return words_of(out)


def calc_flip_reference(pos, own, enemy):
    ref = O.np_calc_flip(np.minimum(pos, 63), own, enemy)
    ref[np.asarray(pos) > 63] = 0
    return ref


def step_reference(black, white, player, status, action):
    """The oracle's step; on the running boards whose action is 64..254 the contract of include/raz.h instead (module docstring)."""
    action = np.asarray(action, dtype=np.uint8)
    off = (action >= 64) & (action != 255)
    b, w, p, s, l = O.np_step(black, white, player, status, np.where(off, 255, action).astype(np.uint8))
    lost = off & (np.asarray(status) == 0)
    assert ((s[lost] & 0x20) != 0).all() and (l[lost] == 0).all()          # (resigned there: the same winner, the board untouched)
    s[lost] = (s[lost] & 0x0f) | 0x10
    return b, w, p, s, l


# ------------------------------------------------------------------------------------------------------------------ inputs
def _frozen(d):
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def inputs(n):
    """Every array of every entry for n boards, seeded by n; read-only, made once.
      black / white (= own / enemy, = d4's x)  disjoint colours at every density from 1/2 down to 1/16, the sparse ones (a quarter of
          the boards) where passes and endings are common; FULL boards (one colour / both) and EMPTY boards (i % 97 in 5, 6, 7);
          own-and-enemy OVERLAP garbage on the boards i % 2048 in [64, 96) of every superblock but the third (so that a wave of a
          sliced kernel meets some in its first and in its last superblock, whatever the grid, and has a superblock without any
          between them) and on every 16th board after the last whole superblock;
      player 1 / 2;  status: 10 % finished (1, 2, 3, also with 0x10 / 0x20);
      action: a legal move on 6 boards of 10, else any square; 3 % 255; 1 % in 64..254;
      pos 0..255;  legal: masks of every density, 0, single bits, all 64 (i % 11 in 0, 1, 2);  rnd: all of uint32;  sym 0..7."""
    rng = np.random.default_rng([20260117, n])
    r64 = lambda: rng.integers(0, 2**64, size=n, dtype=np.uint64)
    i = np.arange(n)
    dens = rng.integers(0, 4, size=n)
    black = r64()
    black[dens <= 1] &= r64()[dens <= 1]
    black[dens == 0] &= r64()[dens == 0]
    white = r64()
    white[dens <= 2] &= r64()[dens <= 2]
    white[dens == 0] &= (r64() | r64())[dens == 0]
    sb = i // 2048
    garbage = np.where(sb < n // 2048, (i % 2048 >= 64) & (i % 2048 < 96) & (sb != 2), i % 16 == 5)
    white[~garbage] &= ~black[~garbage]
    white[garbage] |= (black & (r64() | r64()))[garbage]
    full1, empty, full2 = (i % 97 == 5) & ~garbage, (i % 97 == 6) & ~garbage, (i % 97 == 7) & ~garbage
    black[full1], white[full1] = U(2**64 - 1), U(0)
    black[empty], white[empty] = U(0), U(0)
    white[full2] = ~black[full2]
    overlap = (black & white) != 0                       # (all of the garbage boards but those whose black came out empty)
    player = rng.integers(1, 3, size=n, dtype=np.uint8)
    status = np.where(rng.random(n) < 0.1, rng.choice(np.array([1, 2, 3, 0x11, 0x12, 0x21, 0x22], dtype=np.uint8), size=n), 0).astype(np.uint8)
    own, enemy = np.where(player == 1, black, white), np.where(player == 1, white, black)
    rnd = rng.integers(0, 2**32, size=n, dtype=np.uint32)
    a_legal = pick_kth_reference(O.np_find_correct_moves(own, enemy), rnd)
    action = rng.integers(0, 64, size=n, dtype=np.uint8)
    take = (rng.random(n) < 0.6) & (a_legal != 255)
    action[take] = a_legal[take]
    action[rng.random(n) < 0.03] = 255
    odd = rng.random(n) < 0.01
    action[odd] = rng.integers(64, 255, size=n, dtype=np.uint8)[odd]
    pos = np.where(rng.random(n) < 0.5, rng.integers(0, 64, size=n), rng.integers(0, 256, size=n)).astype(np.uint8)
    legal = r64()
    for k in range(1, 6):
        legal[i % 6 >= k] &= r64()[i % 6 >= k]
    legal[i % 11 == 0] = U(0)
    legal[i % 11 == 1] = U(1) << rng.integers(0, 64, size=n).astype(np.uint64)[i % 11 == 1]
    legal[i % 11 == 2] = U(2**64 - 1)
    sym = rng.integers(0, 8, size=n, dtype=np.uint8)
    return _frozen(dict(black=black, white=white, player=player, status=status, action=action, pos=pos, legal=legal, rnd=rnd, sym=sym,
                        overlap=overlap))


@functools.lru_cache(maxsize=None)
def reference(n):
    """{entry: tuple of expected arrays} for inputs(n); read-only, made once and shared by every test that needs it."""
    x = inputs(n)
    b, w = x["black"], x["white"]
    ref = {"legal_moves": (O.np_find_correct_moves(b, w),), "calc_flip": (calc_flip_reference(x["pos"], b, w),),
           "step": step_reference(b, w, x["player"], x["status"], x["action"]), "score": score_reference(b, w),
           "d4": (d4_reference(b, x["sym"]),), "planes": (planes_reference(b, w),), "pick_kth": (pick_kth_reference(x["legal"], x["rnd"]),)}
    for t in ref.values():
        for a in t:
            a.setflags(write=False)
    return ref


OUTPUT_NAMES = {"legal_moves": ("legal",), "calc_flip": ("flipped",), "step": ("black", "white", "player", "status", "legal"),
                "score": ("winner", "diff"), "d4": ("out",), "planes": ("planes",), "pick_kth": ("action",)}


def call(drv, entry, n, offsets=None):
    x = inputs(n)
    kw = {"offsets": offsets} if offsets else {}
    if entry == "legal_moves":
        out = drv.legal_moves(x["black"], x["white"], **kw)
    elif entry == "calc_flip":
        out = drv.calc_flip(x["pos"], x["black"], x["white"], **kw)
    elif entry == "step":
        out = drv.step(x["black"], x["white"], x["player"], x["status"], x["action"], **kw)
    elif entry == "score":
        out = drv.score(x["black"], x["white"], **kw)
    elif entry == "d4":
        out = drv.d4(x["black"], x["sym"], **kw)
    elif entry == "planes":
        out = drv.planes(x["black"], x["white"], **kw)
    else:
        out = drv.pick_kth(x["legal"], x["rnd"], **kw)
    return out if isinstance(out, tuple) else (out,)


def _compare(entry, n, got, want):
    assert len(got) == len(want), (entry, len(got), len(want))
    for name, g, w in zip(OUTPUT_NAMES[entry], got, want):
        g = np.asarray(g)
        if entry == "planes":
            g = g.reshape(-1, 128)
        assert g.dtype == w.dtype and g.shape == w.shape, (entry, name, n, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.nonzero((g != w).reshape(len(w), -1).any(axis=1))[0] if len(w) else np.zeros(0, dtype=np.int64)
        assert bad.size == 0, (f"{entry}: {name} differs on {bad.size} of {n} boards, first at {bad[:8].tolist()}: "
                               f"got {g[bad[:3]].tolist()}, want {w[bad[:3]].tolist()}")


# ------------------------------------------------------------------------------------------------------------------ the cases
def check_configuration(drv, config):
    """The first thing a process checks: the cap and the forms its variables ask for are in force (config None: a process without
    variables of its own says nothing about the forms, which an earlier test of the same process may have fixed, and the default cap)."""
    if config is None:
        assert drv.max_grid() == DEFAULT_MAX_GRID, drv.max_grid()
        return
    c = CONFIGS[config]
    assert drv.max_grid() == c["max_grid"], (config, drv.max_grid())
    assert drv.forms(N_LOOP) == c["forms"], (config, drv.forms(N_LOOP))
    assert drv.forms(2047) == (0, 0)


def check_iterations(drv, config):
    """The iteration guard: on N_LOOP boards every kernel the configuration is there for goes round its loop >= 3 times on its busiest
    wave and >= 2 on its least busy one - from the cap and the forms THE LIBRARY reports, so that a variable that silently does nothing
    fails here.  Under the default cap every count is 1 (or 0: not launched).  Returns the counts."""
    t = trips(drv.max_grid(), drv.forms(N_LOOP), N_LOOP)
    if config is None:
        assert all(v in ((1, 1), (0, 0)) for v in t.values()), t
        return t
    for k in CONFIGS[config]["looped"]:
        assert t[k][0] >= 3 and t[k][1] >= 2, (config, k, t[k])
    first, last = first_and_last_superblocks(drv.max_grid(), N_LOOP)
    if drv.forms(N_LOOP) != (0, 0):
        ov = np.unique(np.nonzero(inputs(N_LOOP)["overlap"][: 5 * 2048])[0] // 2048)
        assert first <= set(ov.tolist()) and last <= set(ov.tolist()) and 2 not in ov, (first, last, ov)
    return t


def check_entry(drv, entry, n, config=None):
    """One entry on inputs(n) == its reference; on N_LOOP boards in a configuration, with the iteration guard on its kernels."""
    if config is not None and n == N_LOOP:
        t = trips(drv.max_grid(), drv.forms(n), n)
        looped = [k for k in KERNELS_OF[entry] if k in CONFIGS[config]["looped"]]
        assert looped, (entry, config)
        for k in looped:
            assert t[k][0] >= 3 and t[k][1] >= 2, (config, k, t[k])
    _compare(entry, n, call(drv, entry, n), reference(n)[entry])


# every alignment the entries enforce (csrc/raz_sweep.hip raz_*_batch, include/raz.h): (entry, argument, bytes off) that must be refused
REFUSALS = ([("legal_moves", a, 8) for a in ("own", "enemy", "legal")] + [("calc_flip", a, 8) for a in ("own", "enemy", "flipped")]
            + [("calc_flip", "pos", 1)]
            + [("step", a, 8) for a in ("black", "white", "legal")] + [("step", a, k) for a in ("player", "status", "action") for k in (1, 2)]
            + [("score", a, 8) for a in ("black", "white")] + [("score", a, 1) for a in ("winner", "diff")]
            + [("d4", a, 8) for a in ("x", "out")] + [("d4", "sym", 1)])


def check_refusals(drv, n=257):
    """Every misaligned array in turn is refused with RAZ_EINVAL and a message that names the entry, and no output is touched.  (The
    entries compare the pointers on the host, in RAZ_REQUIRE, before the first hipLaunchKernelGGL: a refused call launches nothing.)
    Returns how many calls were refused."""
    x = inputs(n)
    count = 0
    for entry, arg, off in REFUSALS:
        if arg in drv.allocates:
            continue
        try:
            call(drv, entry, n, offsets={arg: off})
        except Refused as r:
            assert r.rc in (None, RAZ_EINVAL), (entry, arg, off, r.rc)
            assert f"raz_{entry}_batch" in r.message and "aligned" in r.message, (entry, arg, off, r.message)
            if r.rc is None:
                assert f"code {RAZ_EINVAL})" in r.message, r.message
            for name, a in r.outputs.items():
                a = np.asarray(a)
                if entry == "step" and name != "legal":
                    assert np.array_equal(a, x[name]), (entry, arg, off, name)
                else:
                    assert (a.view(np.uint8) == SENTINEL).all(), (entry, arg, off, name)
            count += 1
        else:
            raise AssertionError(f"raz_{entry}_batch took {arg} {off} bytes off its alignment")
    return count


def check_step_with_bytes_4_off(drv, n=N_LOOP):
    """player / status / action 4 bytes behind a 16-byte boundary: accepted, and the five arrays equal the aligned call's on the same
    boards (== the reference).  Where the hybrid form is in force this is its demotion to k_step, which then takes ALL the boards -
    pinned by the results alone."""
    aligned = call(drv, "step", n)
    moved = call(drv, "step", n, offsets={"player": 4, "status": 4, "action": 4})
    _compare("step", n, aligned, reference(n)["step"])
    _compare("step", n, moved, reference(n)["step"])
    for a, b in zip(aligned, moved):
        assert np.array_equal(a, b)


def self_check():
    """What the cases take for granted, checked on the references alone."""
    # the d4 restatement == the oracle's flip_vertical / rotate90, 64 random words x 8 symmetries
    orc = O.load()
    rng = np.random.default_rng(64)
    x = rng.integers(0, 2**64, size=64, dtype=np.uint64)
    for s in range(8):
        want = []
        for v in x:
            v = int(v)
            if s & 4:
                v = orc.orc_flip_vertical(v)
            for _ in range(s & 3):
                v = orc.orc_rotate90(v)
            want.append(v)
        assert d4_reference(x, np.full(64, s, dtype=np.uint8)).tolist() == want, s
    assert words_of(bits_of(x)).tolist() == x.tolist() and bits_of(np.array([1 << 9], dtype=np.uint64))[0, 9] == 1
    # pick_kth and score restated == plain Python on a few boards
    z, n = inputs(N_LOOP), N_LOOP
    ref = reference(n)
    for i in list(range(40)) + [n - 1]:
        bits = [s for s in range(64) if int(z["legal"][i]) >> s & 1]
        assert ref["pick_kth"][0][i] == (bits[int(z["rnd"][i]) % len(bits)] if bits else 255), i
        d = bin(int(z["black"][i])).count("1") - bin(int(z["white"][i])).count("1")
        assert ref["score"][1][i] == d and ref["score"][0][i] == (1 if d > 0 else 2 if d < 0 else 3), i
    # the inputs hold what their description says
    st, ac, ov = z["status"], z["action"], z["overlap"]
    assert (z["rnd"] >= 2**31).any() and (z["rnd"] < 2**31).any() and (z["pos"] > 69).any() and (z["pos"] < 64).any()
    assert ((ac >= 64) & (ac < 255) & (st == 0)).sum() > 20 and (ac == 255).sum() > 100 and set(np.unique(z["sym"])) == set(range(8))
    pcl = popcount(z["legal"])
    assert (pcl == 0).any() and (pcl == 1).any() and (pcl == 64).any() and len(np.unique(pcl)) > 40
    assert ov.sum() > 100 and ov[5 * 2048:].any() and not ov[2 * 2048: 3 * 2048].any() and all(ov[k * 2048: (k + 1) * 2048].any() for k in (0, 1, 3, 4))
    discs = popcount(z["black"] | z["white"])
    assert (discs == 64).sum() > n // 60 and (discs == 0).sum() > n // 120 and (ref["score"][1] < 0).any() and (ref["score"][1] == 64).any()
    assert (ref["score"][0] == 3).any() and (ref["pick_kth"][0] == 255).any() and (ref["calc_flip"][0] != 0).sum() > n // 8
    # the step case: passes, natural endings, 0x10 and 0x20 endings, and more than a quarter of the boards moved
    ob, ow, op, os_, ol = ref["step"]
    ran = (st == 0) & (ac < 64)
    moved = ran & ((ob != z["black"]) | (ow != z["white"]))
    assert (moved & (os_ == 0) & (op == z["player"])).sum() > 10, "passes"
    assert (moved & (os_ != 0)).sum() > 10 and not (os_[moved] & 0x30).any(), "natural endings"
    assert ((os_ & 0x10) != 0)[st == 0].sum() > 100 and ((os_ & 0x20) != 0)[st == 0].sum() > 100 and moved.sum() > n // 4, moved.sum()
    assert (moved & ov).any() and (ol[st != 0] == 0).all() and np.array_equal(ob[st != 0], z["black"][st != 0])
    # the launch arithmetic: one trip at most under the default cap at every size of these tests, for every form ...
    for m in SIZES:
        for forms in ((0, 0), (1, 1), (1, 2), (1, 0)):
            assert all(v in ((1, 1), (0, 0)) for v in trips(DEFAULT_MAX_GRID, forms, m).values()), (m, forms)
    # ... and the counts the module docstring quotes
    t = trips(2, (0, 0), N_LOOP)
    assert t["k_legal_moves"] == (6, 5) and t["k_step"] == (6, 5) and t["k_calc_flip"] == (11, 10) and t["k_planes"] == (1319, 1318), t
    assert t["k_pick_kth"] == (21, 20) and t["k_legal_moves_sliced"] == (0, 0), t
    t = trips(2, (1, 1), N_LOOP)
    assert t["k_legal_moves_sliced"] == (3, 2) and t["k_step_sliced"] == (3, 2) and t["k_step_hybrid"] == (0, 0) and t["k_step"] == (1, 1), t
    assert trips(1, (1, 2), N_LOOP)["k_step_hybrid"] == (5, 5) and trips(1, (0, 0), N_LOOP)["k_step"] == (11, 10)
    assert first_and_last_superblocks(2, N_LOOP) == ({0, 1}, {4, 3}) and first_and_last_superblocks(1, N_LOOP) == ({0}, {4})
    # every kernel is looped in some configuration
    assert {k for c in CONFIGS.values() for k in c["looped"]} == {k for ks in KERNELS_OF.values() for k in ks}
