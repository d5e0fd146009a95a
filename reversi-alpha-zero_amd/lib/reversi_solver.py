"""Drop-in for reversi_zero/lib/reversi_solver.py (compiled form: lib/alt/reversi_solver_cython.pyx:40-127), backed by
raz_solve_batch and raz_solve_exact (include/raz.h; kernels in csrc/raz_solver_batch.hip, raz_solver_exact.hip and the header
they share, raz_solver_split.h): the exact end-game solver for one position - `solve`, the reference's signature and answers - or
for arrays of positions at once - `solve_batch`; `solve_exact` / `solve_exact_batch` take deeper positions, and `solve_wld` /
`solve_wld_batch` (raz_solve_wld, csrc/raz_solver_wld.hip) answer who wins for deeper ones still.  Device-only, like the
batched functions of lib/bitboard.py: there is no CPU fallback, and without a GPU the call raises RuntimeError."""
import numpy as np

from .._native import lib, check, tensor_ptr, current_stream_ptr

MAX_EMPTIES = 14   # the library's declared limit: below turn 46 the reference leans on its 30 s wall-clock time-out

EXACT_MAX_EMPTIES = 17   # raz_solve_exact's limit (RAZ_SOLVE_EXACT_MAX_EMPTIES): the full scan's answer, found with bounds passed down

WLD_MAX_EMPTIES = 21   # raz_solve_wld's limit (RAZ_SOLVE_WLD_MAX_EMPTIES): who wins, and the lowest-numbered move of that outcome

SOLVED, NO_MOVE, TOO_MANY_EMPTIES, NOT_A_POSITION = 0, 1, 2, 3


def _player_byte(p):
    return int(getattr(p, "value", p))   # a Player (env/reversi_env.py) or 1 / 2


def _popcount64(x):
    """Set bits per element of an int64 / uint64 device tensor, as an int64 tensor."""
    import torch
    x = x.view(torch.int64).reshape(-1)
    count = torch.zeros_like(x)
    for shift in range(0, 64, 8):
        byte = (x >> shift) & 0xff
        byte = (byte & 0x55) + ((byte >> 1) & 0x55)
        byte = (byte & 0x33) + ((byte >> 2) & 0x33)
        count += (byte & 0x0f) + ((byte >> 4) & 0x0f)
    return count


class ReversiSolver:
    """calculate which is winner. Not estimation by NN!  (lib/reversi_solver.py:17-21)

    An instance owns ONE workspace and hands it to every call, on whatever stream is current: calls through the same instance
    must be ordered on one stream (or synchronised by the caller).  Work on several streams at once takes one instance each."""

    def __init__(self, device=None):
        self._device = device
        self._ws = None   # the workspace of raz_solve_batch: owned here, grown when a batch needs more, reused otherwise
        self._ws_exact = None   # the workspace of raz_solve_exact, likewise
        self._ws_wld = None   # the workspace of raz_solve_wld, likewise

    def _workspace(self, n, device):
        import torch
        least = lib.raz_solve_batch_workspace_bytes(n, MAX_EMPTIES)
        if least == 0:
            raise ValueError(f"raz_solve_batch refuses a batch of {n} positions")
        # above the minimum (one row's worst case) room for whole rows to share a pass: 4 KB a row covers the worst case of 10 empties
        want = least + min(n * 4096, 1 << 31)
        if self._ws is None or self._ws.numel() < want or self._ws.device != device:
            self._ws = torch.empty(want, dtype=torch.uint8, device=device)
        return self._ws

    def solve_batch(self, black, white, next_player, exactly=False):
        """Arrays of positions: `black`, `white` int64 / uint64 device tensors (bit i = square i), `next_player` a uint8 device
        tensor (1 black, 2 white).  Returns device tensors (move int8, score int8, status uint8), one entry per position:
        status 0 = solved - the reference's (move, score), score from the side to move's view; 1 = the side to move has no legal
        move (the reference's (None, None)); 2 = refused, more than 14 empty squares; 3 = not a position (a square of both
        colours, a player byte other than 1 / 2); move = -1 and score = -100 where status != 0.  An answer depends on its
        position and the mode alone, never on the rest of the batch."""
        n, move, score, status = self._check_batch(black, white, next_player, "solve_batch")
        if n:
            ws = self._workspace(n, black.device)
            check(lib.raz_solve_batch(tensor_ptr(black), tensor_ptr(white), tensor_ptr(next_player), n, int(bool(exactly)),
                                      tensor_ptr(move), tensor_ptr(score), tensor_ptr(status), tensor_ptr(ws), ws.numel(), 0,
                                      current_stream_ptr()), "raz_solve_batch")
        return move, score, status

    @staticmethod
    def _check_batch(black, white, next_player, what):
        """The checks of a batch call's arguments; its number of positions and its three outputs (move, score, status)."""
        import torch
        for t in (black, white):
            if t.dtype not in (torch.int64, torch.uint64):
                raise TypeError("bitboard tensors must be int64/uint64")
        if next_player.dtype != torch.uint8:
            raise TypeError("next_player must be a uint8 tensor")
        if not (black.is_cuda and white.is_cuda and next_player.is_cuda):
            raise ValueError(f"{what} is device-only (no CPU fallback)")
        n = black.numel()
        if white.numel() != n or next_player.numel() != n:
            raise ValueError("black, white and next_player must have the same number of elements")
        move, score = (torch.empty(n, dtype=torch.int8, device=black.device) for _ in range(2))
        return n, move, score, torch.empty(n, dtype=torch.uint8, device=black.device)

    def solve_exact_batch(self, black, white, next_player):
        """solve_batch(..., exactly=True) for positions of up to EXACT_MAX_EMPTIES empty squares (raz_solve_exact: the same
        answers, found by a search that passes bounds down): device tensors (move int8, score int8, status uint8); status 2 =
        more than EXACT_MAX_EMPTIES empties.  The call synchronises the current stream (once per group of rounds of the search)."""
        import torch
        n, move, score, status = self._check_batch(black, white, next_player, "solve_exact_batch")
        if n:
            empties = 64 - _popcount64(black.view(torch.int64).reshape(-1) | white.view(torch.int64).reshape(-1))
            deepest = int(torch.where(empties <= EXACT_MAX_EMPTIES, empties, torch.zeros_like(empties)).max())
            want = lib.raz_solve_exact_workspace_bytes(n, deepest)
            if want == 0:
                raise ValueError(f"raz_solve_exact refuses a batch of {n} positions")
            want += min(n * 65536, 1 << 31)   # room for whole rows to share a pass
            ws = self._ws_exact
            if ws is None or ws.numel() < want or ws.device != black.device:
                ws = self._ws_exact = torch.empty(want, dtype=torch.uint8, device=black.device)
            check(lib.raz_solve_exact(tensor_ptr(black), tensor_ptr(white), tensor_ptr(next_player), n, tensor_ptr(move),
                                      tensor_ptr(score), tensor_ptr(status), tensor_ptr(ws), ws.numel(), 0, current_stream_ptr()),
                  "raz_solve_exact")
        return move, score, status

    def solve_wld_batch(self, black, white, next_player):
        """Who wins, for positions of up to WLD_MAX_EMPTIES empty squares (raz_solve_wld): device tensors (move int8, outcome int8,
        status uint8); outcome = +1 / 0 / -1, the sign of the game-theoretic disc difference from the side to move's view, move =
        the lowest-numbered legal move of that outcome; status as solve_batch, 2 = more than WLD_MAX_EMPTIES empties.  The call
        synchronises the current stream (once per group of rounds of the search)."""
        import torch
        n, move, outcome, status = self._check_batch(black, white, next_player, "solve_wld_batch")
        if n:
            empties = 64 - _popcount64(black.view(torch.int64).reshape(-1) | white.view(torch.int64).reshape(-1))
            deepest = int(torch.where(empties <= WLD_MAX_EMPTIES, empties, torch.zeros_like(empties)).max())
            want = lib.raz_solve_wld_workspace_bytes(n, deepest)
            if want == 0:
                raise ValueError(f"raz_solve_wld refuses a batch of {n} positions")
            want += min(n * 65536, 1 << 31)   # room for whole rows to share a pass
            ws = self._ws_wld
            if ws is None or ws.numel() < want or ws.device != black.device:
                ws = self._ws_wld = torch.empty(want, dtype=torch.uint8, device=black.device)
            check(lib.raz_solve_wld(tensor_ptr(black), tensor_ptr(white), tensor_ptr(next_player), n, tensor_ptr(move),
                                    tensor_ptr(outcome), tensor_ptr(status), tensor_ptr(ws), ws.numel(), 0, current_stream_ptr()),
                  "raz_solve_wld")
        return move, outcome, status

    def _solve_one(self, batch_call, black, white, next_player, limit, who):
        """One position through a batch call: (move, score), (None, None) without a legal move, ValueError for what is refused."""
        import torch
        device = torch.device(self._device or "cuda")
        player = _player_byte(next_player)
        if player not in (1, 2):
            raise ValueError(f"next_player must be Player.black / Player.white or 1 / 2, not {next_player!r}")
        m64 = (1 << 64) - 1
        b = torch.from_numpy(np.array([int(black) & m64], dtype=np.uint64).view(np.int64)).to(device)
        w = torch.from_numpy(np.array([int(white) & m64], dtype=np.uint64).view(np.int64)).to(device)
        p = torch.tensor([player], dtype=torch.uint8, device=device)
        move, score, status = (int(t.cpu()[0]) for t in batch_call(b, w, p))
        if status == TOO_MANY_EMPTIES:
            raise ValueError(f"the {who} takes positions of at most {limit} empty squares "
                             f"(this one has {64 - bin((int(black) | int(white)) & m64).count('1')})")
        if status == NOT_A_POSITION:
            raise ValueError("not a position: a square holds a disc of both colours")
        if status == NO_MOVE:
            return None, None
        return move, score

    def solve_exact(self, black, white, next_player):
        """solve(..., exactly=True) for a position of up to EXACT_MAX_EMPTIES empty squares: (move, score) or (None, None)."""
        return self._solve_one(self.solve_exact_batch, black, white, next_player, EXACT_MAX_EMPTIES, "exact solver")

    def solve_wld(self, black, white, next_player):
        """Who wins a position of up to WLD_MAX_EMPTIES empty squares: (move, outcome) or (None, None)."""
        return self._solve_one(self.solve_wld_batch, black, white, next_player, WLD_MAX_EMPTIES, "win/draw/loss solver")

    def solve(self, black, white, next_player, timeout=30, exactly=False):
        """ReversiSolver.solve (lib/alt/reversi_solver_cython.pyx:40-61): (move, score) with score the disc difference from the
        side to move's view, or (None, None) when the side to move has no legal move.  exactly=False is the win/loss mode (every
        node's scan stops at its first winning move), True the full scan.

        `timeout` is accepted and ignored: the reference gives up - (None, None) - when its wall clock runs out, so its answer
        depends on the host's speed; here the answer is a function of the position and the mode alone.  What the reference could
        only try under its time-out is refused instead: more than 14 empty squares raises ValueError, and so does a position
        with a square of both colours."""
        return self._solve_one(lambda b, w, p: self.solve_batch(b, w, p, exactly=exactly), black, white, next_player, MAX_EMPTIES, "solver")
