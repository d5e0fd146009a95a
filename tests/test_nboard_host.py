"""CPU: the NBoard front-end (play_game/nboard.py) on stub players - the protocol's commands and replies, the reader thread's
ping, the command line - and, `needs_reference`, the same scripted session through the unmodified reference's
NBoardProtocolVersion2 with the same stub engine: identical transcripts for every command both implement."""
import io
import queue
import threading
from types import SimpleNamespace

import pytest

from reversi_alpha_zero_amd.agent.player import ActionWithEvaluation, HistoryItem
from reversi_alpha_zero_amd.config import Config, NBoardConfig, PlayConfig, PlayWithHumanConfig
from reversi_alpha_zero_amd.lib.ggf import make_ggf_string
from reversi_alpha_zero_amd.play_game import nboard as NB

GAME = make_ggf_string("b", "w", moves=["F5", "D6"])
SCRIPT = ["nboard 2", "set depth 6", "set depth x", f"set game {GAME}", "go", "move C3/1.5/2", "hint 2", "move pa", "ping 11", "learn",
          "set game " + make_ggf_string("b", "w", moves=["F5"]), "nboard 3", "what is this"]


class StubEngine:
    """What a protocol handler needs of an engine, recording every call; the answers are canned."""

    def __init__(self, go_response, hint_response):
        self.out, self.go_response, self.hint_response, self.handler = [], go_response, hint_response, None

    def reply(self, message):
        self.out.append(message)

    def set_depth(self, n):
        self.out.append(("set_depth", n))

    def set_game(self, gs):
        self.out.append(("set_game", gs.black, gs.white, list(gs.actions), gs.player.name))

    def reset_state(self):
        self.out.append(("reset_state",))

    def move(self, action):
        self.out.append(("move", action))

    def go(self):
        return self.go_response(44, 0.125, 1.5)

    def hint(self, n):
        self.handler.report_hint([self.hint_response(18, 0.5, 30), self.hint_response(20, -0.25, 12), self.hint_response(2, 0.0, 3)][:n])

    def analyze(self):
        return [(0, 0.01, False), (1, -0.2, False), (2, -6.0, True)]


def transcript(module, config, script):
    engine = StubEngine(module.GoResponse, module.HintResponse)
    engine.handler = module.NBoardProtocolVersion2(config, engine)
    for line in script:
        engine.handler.handle_message(line)
    return engine.out


def test_protocol_commands_and_replies_on_a_stub_engine():
    out = transcript(NB, Config(), SCRIPT + ["analyze"])
    assert out[:2] == ["set myname RAZ(default)", "status waiting"]
    assert ("set_depth", "6") in out and ("set_depth", "x") not in out
    init = (0x0000000810000000, 0x0000001008000000)
    assert ("set_game", *init, [44, 29], "black") in out and ("set_game", *init, [44], "black") in out
    assert out.count(("reset_state",)) == 1 and out.index(("reset_state",)) > out.index(("set_game", *init, [44], "black"))
    go = out.index("=== F5/1.25/1.5")
    assert out[go - 1] == "status thinking..." and out[go + 1] == "status waiting"
    assert ("move", 18) in out and ("move", None) in out
    h = out.index("status thinkng hint...")
    assert out[h + 1:h + 4] == ["search C5 -0.25 0 12", "search C3 0.5 0 30", "status waiting"]   # the last one is the best
    assert "pong 11" in out and "learned" in out
    assert out[-5:] == ["status analyzing...", "analysis 0 0.1", "analysis 1 -2.0", "analysis 2 -6.0", "status waiting"]


@pytest.mark.needs_reference
def test_transcripts_equal_the_reference_handler():
    import ref_harness as rh
    rh.install()
    import reversi_zero.play_game.nboard as ref
    from reversi_zero.config import Config as RefConfig
    assert "analyze" not in " ".join(SCRIPT)
    mine, theirs = transcript(NB, Config(), SCRIPT), transcript(ref, RefConfig(), SCRIPT)
    assert mine == theirs and len(mine) == 19
    assert transcript(ref, RefConfig(), ["analyze"]) == []   # the command the reference leaves as `pass`


@pytest.mark.needs_reference
def test_play_with_human_and_nboard_sections_equal_the_reference():
    import ref_harness as rh
    rh.install()
    import reversi_zero.config as R
    assert vars(PlayWithHumanConfig()) == vars(R.PlayWithHumanConfig()) and vars(NBoardConfig()) == vars(R.NBoardConfig())
    mine, theirs = PlayConfig(), R.PlayConfig()
    PlayWithHumanConfig().update_play_config(mine)
    R.PlayWithHumanConfig().update_play_config(theirs)
    assert vars(mine) == vars(theirs)
    assert (mine.noise_eps, mine.change_tau_turn, mine.parallel_search_num, mine.resign_threshold) == (0, 0, 8, None)
    c = Config()
    assert isinstance(c.play_with_human, PlayWithHumanConfig) and isinstance(c.nboard, NBoardConfig)
    c.update({"nboard": {"my_name": "X"}, "play_with_human": {"parallel_search_num": 2}})
    assert c.nboard.my_name == "X" and c.nboard.hint_callback_per_sim == 10 and c.play_with_human.parallel_search_num == 2


def test_sections_without_the_reference():
    assert vars(NBoardConfig()) == dict(my_name="RAZ", read_stdin_timeout=0.1, simulation_num_per_depth_about=20, hint_callback_per_sim=10)
    pc = PlayConfig()
    PlayWithHumanConfig().update_play_config(pc)
    assert (pc.noise_eps, pc.change_tau_turn, pc.parallel_search_num, pc.resign_threshold, pc.use_newest_next_generation_model) == (0, 0, 8, None, True)


# ---- the engine on a stub player ----------------------------------------------------------------------------------------------
class StubPlayer:
    """ReversiPlayer's interface as the engine uses it: the lowest legal square, with a thinking history made up from it."""

    def __init__(self, wait_for_stop=False):
        self.history, self.stop_requested, self.started, self.wait_for_stop = {}, threading.Event(), threading.Event(), wait_for_stop
        self.callbacks = 0

    def action_with_evaluation(self, own, enemy, callback_in_mtcs=None):
        from reversi_alpha_zero_amd.lib.bitboard import find_correct_moves
        legal = find_correct_moves(own, enemy)
        moves = [a for a in range(64) if (legal >> a) & 1]
        values, visits = [0.0] * 64, [0.0] * 64
        for k, a in enumerate(moves):
            values[a], visits[a] = 0.5 - 0.125 * k, float(10 + k)   # the LAST legal move is the most visited
        if callback_in_mtcs:
            callback_in_mtcs.callback(values, [v / 2 for v in visits])
            self.callbacks += 1
        self.started.set()
        if self.wait_for_stop:
            assert self.stop_requested.wait(30), "no ping reached the search"
        self.history[(own, enemy)] = HistoryItem(moves[0], None, values, visits, None, None)
        return ActionWithEvaluation(moves[0], visits[moves[0]], values[moves[0]])

    def ask_thought_about(self, own, enemy):
        return self.history.get((own, enemy))

    def stop_thinking(self):
        self.stop_requested.set()


class StubbedEngine(NB.NBoardEngine):
    players = []

    def create_player(self):
        self.players.append(StubPlayer(wait_for_stop=getattr(self, "wait_for_stop", False)))
        return self.players[-1]


def _config():
    c = Config()
    c.nboard.read_stdin_timeout = 0.01
    return c


def test_engine_session_on_in_memory_streams():
    out = io.StringIO()
    script = ["nboard 2", f"set game {GAME}", "go", "move C3", "hint 2", "ping 4", "learn", "set depth 10"]
    StubbedEngine.players = []
    engine = StubbedEngine(_config(), stdin=io.StringIO("\n".join(script) + "\n"), stdout=out, model=object())
    engine.start()
    lines = out.getvalue().splitlines()
    assert lines[0] == "set myname RAZ(default)"
    first = next(x for x in lines if x.startswith("==="))
    assert first.startswith("=== C3/5.0/")   # black to move after F5 D6: the stub's lowest legal square, its value x10
    searches = [x for x in lines if x.startswith("search")]
    assert len(searches) == 4 and searches[1] == searches[3].replace(searches[3].split()[-1], str(int(searches[3].split()[-1]) // 2))
    assert float(searches[3].split()[2]) < float(searches[2].split()[2]) and int(searches[3].split()[4]) > int(searches[2].split()[4])
    assert lines[-2:] == ["pong 4", "learned"] and engine.players[-1].callbacks == 1
    assert engine.game_state.actions == [44, 29, 18] and engine.env.turn == 3
    assert engine.play_config.required_visit_to_decide_action == 200 and engine.play_config.thinking_loop == 5
    assert len(engine.players) == 1   # (a game set at its third move keeps the tree)
    # `go` when the side to move is not the one NBoard expects - the opponent had to pass and no pass entry was sent (nboard.py:115-116)
    engine.turn_of_nboard = NB.Player.white if engine.env.next_player == NB.Player.black else NB.Player.black
    assert engine.go() == NB.GoResponse(None, 0, 0)


class _Feed:
    """A stream whose lines arrive when the test says so."""

    def __init__(self):
        self.q = queue.Queue()

    def readline(self):
        return self.q.get()


def test_ping_on_the_reader_thread_stops_a_running_search():
    feed, out = _Feed(), io.StringIO()
    StubbedEngine.players = []
    StubbedEngine.wait_for_stop = True
    try:
        engine = StubbedEngine(_config(), stdin=feed, stdout=out, model=object())
        player = engine.players[-1]

        def script():
            feed.q.put("ping 1\n")   # no search runs: answered, nothing to stop
            feed.q.put(f"set game {make_ggf_string(moves=['F5', 'D6', 'C3'])}\n")
            feed.q.put("go\n")
            assert player.started.wait(30)
            assert not player.stop_requested.is_set()
            feed.q.put("ping 2\n")
            feed.q.put("")
        t = threading.Thread(target=script)
        t.start()
        engine.start()
        t.join()
    finally:
        StubbedEngine.wait_for_stop = False
    lines = out.getvalue().splitlines()
    assert player.stop_requested.is_set() and not engine.thinking
    assert lines[0] == "pong 1" and lines[-1] == "pong 2" and any(x.startswith("=== ") for x in lines[1:-1])


def test_command_line_names_the_program(capsys):
    with pytest.raises(SystemExit):
        NB.main(["--help"])
    assert "reversi_alpha_zero_amd.play_game.nboard" in capsys.readouterr().out
