"""Training rows on the device, straight from the self-play outbox (csrc/raz_replay.hip; include/raz.h raz_train_rows_count /
raz_train_rows_fill).

The `self` worker writes a finished game as ~0.7 MB of play_*.json text and the `opt` worker parses that text back into 273 bytes a
row (lib/data_helper.pack_game_data) for the GPU the records came from.  rows_from_outbox makes the same packed rows - bit for bit -
from the engine's record arrays where they lie, and DeviceReplay keeps the window of games the play-data directory would hold
(play_data.nb_game_in_file x play_data.max_file_num, worker/self_play.py:209-217) as one data set the trainer reads in place.
The files stay what the reference's own consumers read; nothing here replaces them."""
import ctypes

import numpy as np

from .._native import check, current_stream_ptr, lib, tensor_ptr


def _outbox_tensors(headers, root_n, summary, done):
    """The shapes, element types and device of an outbox as SelfPlayEngine.pack_records / play_continuous hand it out, checked
    BEFORE a pointer is taken (the kernels get bare pointers and two numbers).  Returns (games, plies)."""
    import torch
    for name, t in (("headers", headers), ("root_n", root_n), ("summary", summary)) + ((("done", done),) if done is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"rows_from_outbox: {name} must be a torch tensor, not {type(t).__name__}")
        if not t.is_cuda:
            raise ValueError("rows_from_outbox is device-only (no CPU fallback): the file route is lib/data_helper.pack_game_data")
        if t.device != headers.device:
            raise ValueError(f"rows_from_outbox: {name} is on {t.device}, headers on {headers.device}")
    if headers.dtype != torch.uint8 or headers.dim() != 3 or headers.shape[2] != 48:
        raise TypeError(f"rows_from_outbox: headers must be uint8 [games, plies, 48], not {headers.dtype} {tuple(headers.shape)}")
    G, plies = int(headers.shape[0]), int(headers.shape[1])
    if root_n.dtype not in (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ()) or tuple(root_n.shape) != (G, plies, 64):
        raise TypeError(f"rows_from_outbox: root_n must be int32 [{G}, {plies}, 64], not {root_n.dtype} {tuple(root_n.shape)}")
    if summary.dtype != torch.uint8 or tuple(summary.shape) != (G, 32):
        raise TypeError(f"rows_from_outbox: summary must be uint8 [{G}, 32], not {summary.dtype} {tuple(summary.shape)}")
    if done is not None and (done.dtype != torch.uint8 or tuple(done.shape) != (G,)):
        raise TypeError(f"rows_from_outbox: done must be uint8 [{G}], not {done.dtype} {tuple(done.shape)}")
    return G, plies


def rows_from_outbox(headers, root_n, summary, done=None, *, change_tau_turn, save_policy_of_tau_1):
    """The trainer's packed rows of the games of an outbox, in outbox (= game id) order: (own int64[R], enemy int64[R], policy
    float32[R, 64], z int8[R], row_offset int32[games + 1]), all on the outbox's device; the rows of game g are
    [row_offset[g], row_offset[g + 1]).  done (optional, uint8[games]): games whose flag is 0 have no rows yet.
    Bit for bit what pack_game_data makes of the play_*.json text of the same games.  Waits for the device once (the row count)."""
    import torch
    G, plies = _outbox_tensors(headers, root_n, summary, done)
    dev = headers.device
    with torch.cuda.device(dev):
        row_offset = torch.empty(G + 1, dtype=torch.int32, device=dev)
        total = ctypes.c_uint64(0)
        if G and plies == 0:
            raise ValueError("rows_from_outbox: an outbox of games without plies")
        check(lib.raz_train_rows_count(tensor_ptr(headers) if G else None, tensor_ptr(summary) if G else None,
                                       tensor_ptr(done) if (done is not None and G) else None, G, max(plies, 1), tensor_ptr(row_offset),
                                       ctypes.byref(total), current_stream_ptr()), "raz_train_rows_count")
        R = int(total.value)
        own = torch.empty(R, dtype=torch.int64, device=dev)
        enemy = torch.empty(R, dtype=torch.int64, device=dev)
        policy = torch.empty((R, 64), dtype=torch.float32, device=dev)
        z = torch.empty(R, dtype=torch.int8, device=dev)
        if R:
            check(lib.raz_train_rows_fill(tensor_ptr(headers), tensor_ptr(root_n), tensor_ptr(summary), tensor_ptr(done) if done is not None else None,
                                          G, plies, int(change_tau_turn), int(bool(save_policy_of_tau_1)), tensor_ptr(row_offset), R,
                                          tensor_ptr(own), tensor_ptr(enemy), tensor_ptr(policy), tensor_ptr(z), current_stream_ptr()),
                  "raz_train_rows_fill")
    return own, enemy, policy, z, row_offset


def games_to_drop(first_game, games, nb_game_in_file, max_file_num):
    """The window of remove_play_data (worker/self_play.py:209-217) on game numbers alone: the replay holds the `games` consecutive
    games first_game, first_game + 1, ... (numbered in arrival order from 0; first_game is a multiple of nb_game_in_file).  A GROUP is
    what one play file holds: the nb_game_in_file games k * nb .. (k + 1) * nb - 1.  At most max_file_num WHOLE groups are kept - the
    oldest go first, whole - and behind them the games of the group that is still filling up (the worker's buffer, its next file).
    Returns how many of the oldest games leave (a multiple of nb_game_in_file)."""
    nb, keep = int(nb_game_in_file), int(max_file_num)
    if nb < 1 or keep < 1:
        raise ValueError("nb_game_in_file and max_file_num must be >= 1")
    if first_game % nb:
        raise ValueError("the replay's first game must start a group")
    whole = (first_game + games) // nb - first_game // nb
    return max(0, whole - keep) * nb


class DeviceReplay:
    """The play-data directory as one packed data set in HBM: add() appends the rows of finished games, the window keeps at most
    max_file_num groups of nb_game_in_file consecutive games (games_to_drop), dataset() is what OptimizeWorker(replay=...) trains on.
    (A game without a single row - no file route game is one - still counts as a game of its group.)"""

    def __init__(self, nb_game_in_file, max_file_num, change_tau_turn, save_policy_of_tau_1, device="cuda:0"):
        games_to_drop(0, 0, nb_game_in_file, max_file_num)   # (validates the two numbers)
        self.nb_game_in_file, self.max_file_num = int(nb_game_in_file), int(max_file_num)
        self.change_tau_turn, self.save_policy_of_tau_1 = int(change_tau_turn), bool(save_policy_of_tau_1)
        self.device = device
        self.first_game = 0                           # arrival number of the oldest game held
        self._game_rows = np.zeros(0, dtype=np.int64)   # rows of every game held, oldest first
        self._parts = []                              # [(own, enemy, policy, z)] device tensors, oldest first
        self.version = 0

    @classmethod
    def from_config(cls, config, device="cuda:0"):
        pd = config.play_data
        if pd.drop_draw_game_rate:
            raise ValueError("play_data.drop_draw_game_rate > 0: the files then leave drawn games out, the device replay keeps every game")
        return cls(pd.nb_game_in_file, pd.max_file_num, config.play.change_tau_turn, pd.save_policy_of_tau_1, device)

    @property
    def games(self):
        return len(self._game_rows)

    @property
    def rows(self):
        return int(self._game_rows.sum())

    def add(self, headers, root_n, summary, done=None):
        """Append the games of an outbox (in its order); returns the number of rows added.  Games whose done flag is 0 are taken as
        games without rows: add finished outboxes."""
        import torch
        own, enemy, policy, z, row_offset = rows_from_outbox(headers, root_n, summary, done, change_tau_turn=self.change_tau_turn,
                                                             save_policy_of_tau_1=self.save_policy_of_tau_1)
        if torch.device(self.device) != own.device:
            raise ValueError(f"the replay lives on {self.device}, the outbox on {own.device}")
        per_game = np.diff(row_offset.cpu().numpy().astype(np.int64))
        if not len(per_game):
            return 0
        if len(own):
            self._parts.append((own, enemy, policy, z))
        self._game_rows = np.concatenate([self._game_rows, per_game])
        drop = games_to_drop(self.first_game, self.games, self.nb_game_in_file, self.max_file_num)
        self._drop_front(drop)
        self.version += 1
        return int(per_game.sum())

    def _drop_front(self, games):
        rows = int(self._game_rows[:games].sum())
        self._game_rows = self._game_rows[games:]
        self.first_game += games
        while rows and self._parts:
            n = len(self._parts[0][0])
            if n <= rows:
                self._parts.pop(0)
                rows -= n
            else:
                self._parts[0] = tuple(t[rows:] for t in self._parts[0])   # (views: the storage goes with the next dataset())
                rows = 0

    def dataset(self):
        """(own int64[R], enemy int64[R], policy float32[R, 64], z int8[R]): contiguous device tensors, the games in arrival order.
        The tensors are the replay's own until the next add(): train on them, do not write to them."""
        import torch
        if len(self._parts) != 1 or self._parts[0][0].storage_offset():
            if self._parts:
                self._parts = [tuple(torch.cat([p[i] for p in self._parts]) for i in range(4))]
            else:
                dev = self.device
                self._parts = [(torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
                                torch.empty((0, 64), dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.int8, device=dev))]
        return self._parts[0]
