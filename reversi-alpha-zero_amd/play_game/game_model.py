"""The observer model of a game against a person - drop-in for reversi_zero/play_game/game_model.py:16-113 on this package's
ReversiPlayer.  A front-end registers observers, starts a game, forwards the person's clicks to move() and asks for move_by_ai()
on GameEvent.ai_move.  (The reference's wx window, play_game/gui.py, is not built.)"""
import enum
from logging import getLogger

from ..agent.player import ReversiPlayer
from ..env.reversi_env import Player, ReversiEnv
from ..lib.bitboard import find_correct_moves
from .common import load_model

logger = getLogger(__name__)

GameEvent = enum.Enum("GameEvent", "update ai_move over pass")


class PlayWithHuman:
    def __init__(self, config, model=None):
        """model: a loaded ReversiModel (None: play_game.common.load_model(config), as the reference)."""
        self.config = config
        self.human_color = None
        self.observers = []
        self.env = ReversiEnv().reset()
        self.model = model if model is not None else self._load_model()
        self.ai = None
        self.last_evaluation = None
        self.last_history = None

    def add_observer(self, observer_func):
        self.observers.append(observer_func)

    def notify_all(self, event):
        for observer in self.observers:
            observer(event)

    def start_game(self, human_is_black):
        self.human_color = Player.black if human_is_black else Player.white
        self.env = ReversiEnv().reset()
        self.ai = ReversiPlayer(self.config, self.model)

    def play_next_turn(self):
        self.notify_all(GameEvent.update)
        if self.over:
            self.notify_all(GameEvent.over)
        elif self.next_player != self.human_color:
            self.notify_all(GameEvent.ai_move)

    @property
    def over(self):
        return self.env.done

    @property
    def next_player(self):
        return self.env.next_player

    @staticmethod
    def _square(px, py):
        return int(py * 8 + px)   # left top = (0, 0), right bottom = (7, 7)

    def stone(self, px, py):
        bit = 1 << self._square(px, py)
        if self.env.board.black & bit:
            return Player.black
        if self.env.board.white & bit:
            return Player.white
        return None

    @property
    def number_of_black_and_white(self):
        return self.env.observation.number_of_black_and_white

    def available(self, px, py):
        pos = self._square(px, py)
        if not 0 <= pos < 64:
            return False
        own, enemy = self.env.board.black, self.env.board.white
        if self.human_color == Player.white:
            own, enemy = enemy, own
        return find_correct_moves(own, enemy) & (1 << pos)

    def move(self, px, py):
        pos = self._square(px, py)
        assert 0 <= pos < 64
        if self.next_player != self.human_color:
            return False
        self.env.step(pos)

    def _load_model(self):
        return load_model(self.config)

    def move_by_ai(self):
        if self.next_player == self.human_color:
            return False
        own, enemy = self.get_state_of_next_player()
        action = self.ai.action(own, enemy)
        self.env.step(action)
        self.last_history = self.ai.ask_thought_about(own, enemy)
        if self.last_history is not None:   # (a move the end-game solver decided has no search history)
            self.last_evaluation = self.last_history.values[self.last_history.action]
        logger.debug(f"evaluation by ai={self.last_evaluation}")

    def get_state_of_next_player(self):
        return self.env.get_own_and_enemy()
