"""The NBoard engine - drop-in for reversi_zero/play_game/nboard.py:23-333 on this package's ReversiPlayer.

    python -m reversi_alpha_zero_amd.play_game.nboard -c config/<file>.yml

is the program NBoard (http://www.orbanova.com/nboard/) is pointed at; it speaks NBoard's protocol version 2 on stdin / stdout.
Commands and replies are the reference's (nboard.py:154-333: nboard, set depth, set game, move, hint, go, ping, learn) with two
differences:
  1. a `ping` that arrives while a search runs stops that search (ReversiPlayer.stop_thinking) - the reference's ping handler has
     the call commented out and relies on push_callback alone; here the reader thread does it, and only while a search runs;
  2. `analyze`, which the reference leaves as `pass`, is implemented: the game as set so far goes through lib/analysis.GameAnalyzer
     (every position searched at once on the device), and one `analysis {movesMade} {eval}` line is sent per position, movesMade
     ascending, eval x10 as `go` scales it, from the point of view of the side to move (the only one the protocol text defines);
     positions where the game is over report the final disc difference.
The engine takes its input and output streams as arguments, so a test needs no real stdin."""
import queue
import re
import sys
import threading
from collections import namedtuple
from logging import FileHandler, StreamHandler, getLogger
from time import time

from ..agent.player import CallbackInMCTS, ReversiPlayer
from ..env.reversi_env import Player, ReversiEnv
from ..lib.ggf import convert_action_to_move, convert_move_to_action, convert_to_bitboard_and_actions, parse_ggf

logger = getLogger(__name__)

GameState = namedtuple("GameState", "black white actions player")
GoResponse = namedtuple("GoResponse", "action eval time")
HintResponse = namedtuple("HintResponse", "action value visit")


def start(config, stdin=None, stdout=None):
    config.play_with_human.update_play_config(config.play)
    root_logger = getLogger()
    for h in list(root_logger.handlers):   # stdout belongs to the protocol
        if isinstance(h, StreamHandler) and not isinstance(h, FileHandler):
            root_logger.removeHandler(h)
    logger.info(f"config type={config.type}")
    NBoardEngine(config, stdin=stdin, stdout=stdout).start()
    logger.info("finish nboard")


class LineReader:
    """A thread that reads lines of a stream into a queue, so that the engine can look at a line the moment it arrives
    (push_callback, on the reader's thread) and take it up when it is free (readline, with a timeout)."""

    def __init__(self, stream):
        self.stream, self.lines, self.closed, self.thread = stream, queue.Queue(), False, None

    def start(self, push_callback=None):
        def run():
            try:
                for line in iter(self.stream.readline, ""):
                    if push_callback:
                        push_callback(line)
                    self.lines.put(line)
            finally:
                self.closed = True
        self.thread = threading.Thread(target=run, name="nboard-stdin", daemon=True)
        self.thread.start()

    def readline(self, timeout):
        try:
            return self.lines.get(timeout=timeout)
        except queue.Empty:
            return None

    @property
    def drained(self):
        return self.closed and self.lines.empty()


class NBoardEngine:
    def __init__(self, config, stdin=None, stdout=None, model=None, device="cuda:0"):
        """model: a loaded ReversiModel / net (None: play_game.common.load_model(config), as the reference)."""
        self.config = config
        self.stdout = stdout if stdout is not None else sys.stdout
        self.reader = LineReader(stdin if stdin is not None else sys.stdin)
        self.handler = NBoardProtocolVersion2(config, self)
        self.running = False
        self.nc = self.config.nboard
        self.device = device
        self.env = ReversiEnv().reset()
        if model is None:
            from .common import load_model
            model = load_model(self.config)
        self.model = model
        self.play_config = self.config.play
        self.player = self.create_player()
        self.turn_of_nboard = None
        self.game_state = GameState(self.env.board.black, self.env.board.white, [], Player.black)
        self.thinking = False
        self.analyzer = None

    def create_player(self):
        logger.debug("create new ReversiPlayer()")
        return ReversiPlayer(self.config, self.model, self.play_config, enable_resign=False,
                             mtcs_info=ReversiPlayer.create_mtcs_info(device=self.device))

    def start(self):
        self.running = True
        self.reader.start(push_callback=self.push_callback)
        while self.running and not self.reader.drained:
            message = self.reader.readline(self.nc.read_stdin_timeout)
            if message is None:
                continue
            message = message.strip()
            logger.debug(f"> {message}")
            self.handler.handle_message(message)

    def push_callback(self, message):
        # note: called on the reader's thread
        if message.startswith("ping") and self.thinking:   # interrupt
            self.stop_thinkng()

    def stop(self):
        self.running = False

    def reply(self, message):
        logger.debug(f"< {message}")
        self.stdout.write(message + "\n")
        self.stdout.flush()

    def stop_thinkng(self):   # (the reference's spelling)
        self.player.stop_thinking()

    def set_depth(self, n):
        try:
            n = int(n)
        except ValueError:
            return
        pc = self.play_config
        pc.required_visit_to_decide_action = n * self.nc.simulation_num_per_depth_about
        pc.thinking_loop = min(30, int(pc.required_visit_to_decide_action * 5 / pc.simulation_num_per_move))
        self.analyzer = None   # (built from the play config)
        logger.info(f"set required_visit_to_decide_action to {pc.required_visit_to_decide_action}")

    def reset_state(self):
        self.player = self.create_player()

    def set_game(self, game_state):
        self.env.reset()
        self.env.update(game_state.black, game_state.white, game_state.player)
        self.turn_of_nboard = game_state.player
        self.game_state = GameState(game_state.black, game_state.white, [], game_state.player)
        for action in game_state.actions:
            self.move(action)

    def _change_turn(self):
        if self.turn_of_nboard:
            self.turn_of_nboard = Player.black if self.turn_of_nboard == Player.white else Player.white

    def move(self, action):
        self._change_turn()
        self.game_state.actions.append(action)
        if action is not None:
            self.env.step(action)

    def _search(self, callback_in_mtcs=None):
        """(own, enemy, the player's answer, its thinking history or None) of a search of the current position."""
        states = self.env.get_own_and_enemy()
        self.thinking = True
        try:
            answer = self.player.action_with_evaluation(*states, callback_in_mtcs=callback_in_mtcs)
        finally:
            self.thinking = False
        return answer, self.player.ask_thought_about(*states)

    def go(self):
        if self.env.next_player != self.turn_of_nboard:
            return GoResponse(None, 0, 0)
        start_time = time()
        answer, item = self._search()
        # (a move the end-game solver decided has no thinking history: its value is the solver's)
        evaluation = item.values[answer.action] if item is not None and answer.action is not None else answer.q
        return GoResponse(answer.action, evaluation, time() - start_time)

    def hint(self, n_hint):
        def hint_report_callback(values, visits):
            ranked = sorted(enumerate(visits), key=lambda x: -x[1])[:n_hint]
            self.handler.report_hint([HintResponse(action, values[action], visit) for action, visit in ranked if visit > 0])

        answer, item = self._search(CallbackInMCTS(self.nc.hint_callback_per_sim, hint_report_callback))
        if item is not None:
            hint_report_callback(item.values, item.visit)
        elif answer.action is not None:
            self.handler.report_hint([HintResponse(answer.action, answer.q, answer.n)])

    def analyze(self):
        """[(moves_made, eval)] of the game as set so far: eval from the side to move's view - the best move's value where the
        position was searched, the final disc difference where the game is over."""
        from ..lib.analysis import GameAnalyzer
        if self.analyzer is None:
            self.analyzer = GameAnalyzer(self.config, self.model, self.play_config, slots=128, device=self.device)
        gs = self.game_state
        positions = self.analyzer.analyze([(gs.black, gs.white, gs.player.value, list(gs.actions))])[0]
        return [(d["moves_made"], float(d["disc_diff"]) if "disc_diff" in d and "eval" not in d else d.get("eval", 0.0), d["state"] == "over")
                for d in positions]


class NBoardProtocolVersion2:
    def __init__(self, config, engine):
        self.config = config
        self.engine = engine
        self.handlers = [
            (re.compile(r'nboard ([0-9]+)'), self.nboard),
            (re.compile(r'set depth ([0-9]+)'), self.set_depth),
            (re.compile(r'set game (.+)'), self.set_game),
            (re.compile(r'move ([^/]+)(/[^/]*)?(/[^/]*)?'), self.move),
            (re.compile(r'hint ([0-9]+)'), self.hint),
            (re.compile(r'go'), self.go),
            (re.compile(r'ping ([0-9]+)'), self.ping),
            (re.compile(r'learn'), self.learn),
            (re.compile(r'analyze'), self.analyze),
        ]

    def handle_message(self, message):
        for regexp, func in self.handlers:
            match = regexp.match(message)
            if match:
                func(*match.groups())
                return
        logger.debug(f"ignore message: {message}")

    def nboard(self, version):
        if version != "2":
            logger.warning(f"UNKNOWN NBoard Version {version}!!!")
        self.engine.reply(f"set myname {self.config.nboard.my_name}({self.config.type})")
        self.tell_status("waiting")

    def set_depth(self, depth):
        """Optional: the engine's midgame search depth; mapped to required_visit_to_decide_action."""
        self.engine.set_depth(depth)

    def set_game(self, ggf_str):
        """All further commands relate to the position at the end of the given game, in GGF format (BO, B, W matter)."""
        ggf = parse_ggf(ggf_str)
        black, white, actions = convert_to_bitboard_and_actions(ggf)
        player = Player.black if ggf.BO.color == "*" else Player.white
        self.engine.set_game(GameState(black, white, actions, player))
        if len(actions) <= 1:   # a game at its first moves: forget the search tree of the last one
            self.engine.reset_state()

    def move(self, move, evaluation, time_sec):
        """All further commands relate to the position after the given move ("F5", or "PA"); no response."""
        self.engine.move(convert_move_to_action(move))

    def hint(self, n):
        """Evaluations of about the top n moves: `search {pv} {eval} 0 {depth}` lines, also while the search runs; the last is the best."""
        self.tell_status("thinkng hint...")
        self.engine.hint(int(n))
        self.tell_status("waiting")

    def report_hint(self, hint_list):
        for hint in reversed(hint_list):
            self.engine.reply(f"search {convert_action_to_move(hint.action)} {hint.value} 0 {int(hint.visit)}")

    def go(self):
        """The move the engine would play: `=== {move}/{eval}/{time}`; the board is not updated (NBoard sends `move`)."""
        self.tell_status("thinking...")
        gr = self.engine.go()
        self.engine.reply(f"=== {convert_action_to_move(gr.action)}/{gr.eval * 10}/{gr.time}")
        self.tell_status("waiting")

    def ping(self, n):
        """Synchronisation before the position changes: `pong n`.  (A running search was stopped when the line arrived.)"""
        self.engine.reply(f"pong {n}")

    def learn(self):
        self.engine.reply("learned")

    def analyze(self):
        """Retrograde analysis of the current game: `analysis {movesMade} {eval}` per position, movesMade ascending (0 = the start
        position; passes count)."""
        self.tell_status("analyzing...")
        for moves_made, evaluation, over in self.engine.analyze():
            self.engine.reply(f"analysis {moves_made} {evaluation if over else evaluation * 10}")
        self.tell_status("waiting")

    def tell_status(self, status):
        self.engine.reply(f"status {status}")


def main(argv=None):
    import argparse
    from ..config import load_config
    parser = argparse.ArgumentParser(prog="python -m reversi_alpha_zero_amd.play_game.nboard", description="NBoard engine (protocol version 2)")
    parser.add_argument("-c", "--config", help="a config yml (config/*.yml of the reference loads unchanged)")
    parser.add_argument("--log", help="log file (stdout is the protocol's)")
    args = parser.parse_args(argv)
    if args.log:
        import logging
        logging.basicConfig(filename=args.log, level=logging.DEBUG)
    start(load_config(args.config))


if __name__ == "__main__":
    main()
