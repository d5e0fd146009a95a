"""GGF side-output of self-play (reversi_zero/lib/ggf.py:35-100): move <-> action naming and the
game string.  Note the reference's naming is transposed w.r.t. standard Othello: the LETTER is the
row and the DIGIT the column ("A1" = 0, "F5" = 44, test/lib/test_ggf.py:32-43)."""
from datetime import datetime


def convert_move_to_action(move_str):
    if move_str[:2].lower() == "pa":
        return None
    pos = move_str.lower()
    return (ord(pos[0]) - ord("a")) * 8 + int(pos[1]) - 1


def convert_action_to_move(action):
    if action is None:
        return "PA"
    return chr(ord("A") + action // 8) + str(action % 8 + 1)


def make_ggf_string(black_name=None, white_name=None, dt=None, moves=None, result=None, think_time_sec=60):
    dt = dt or datetime.utcnow()
    move_list = "".join(("B[%s]" if i % 2 == 0 else "W[%s]") % m for i, m in enumerate(moves or []))
    return ("(;GM[Othello]PC[RAZSelf]DT[%s]PB[%s]PW[%s]RE[%s]TI[%s]TY[8]"
            "BO[8 ---------------------------O*------*O--------------------------- *]%s;)") % (
        dt.strftime("%Y.%m.%d_%H:%M:%S.%Z"), black_name or "black", white_name or "white", result or "?",
        f"{think_time_sec // 60}:{think_time_sec % 60}", move_list)


# ---- reading a game (the GGF format, https://skatgame.net/mburo/ggsa/ggf) -------------------------------------------------------
# A game is "(;" + properties + ";)", a property is NAME[value]; the ones a position needs are BO[8 <64 squares> <colour>] - the
# squares row by row, '*' black, 'O' white, '-' empty, then the side to move - and the moves B[..] / W[..] in play order, each value
# "<square>" or "<square>/<eval>/<time>", "PA" (any case, "PASS" too) for a pass.  Property names are matched in either case.
from collections import namedtuple
import re

GGF = namedtuple("GGF", "BO MOVES")
BO = namedtuple("BO", "board_type square_cont color")   # color: '*' black to move, 'O' white
MOVE = namedtuple("MOVE", "color pos")                  # color 'B' / 'W', pos like "F5" or "PA"

_PROPERTY = re.compile(r"([A-Za-z]+)\[([^\]]*)\]")
_SQUARE = re.compile(r"[a-h][1-8]$")


def parse_ggf(text):
    """GGF(BO, MOVES) of one game string; ValueError where it holds no usable 8x8 position or a move that names no square."""
    bo, moves = None, []
    for name, value in _PROPERTY.findall(text):
        name = name.upper()
        if name == "BO":
            fields = value.split()
            if len(fields) != 3:
                raise ValueError(f"GGF: BO[{value}] is not '<size> <squares> <colour>'")
            bo = BO(*fields)
            if bo.board_type != "8" or len(bo.square_cont) != 64 or set(bo.square_cont) - set("*O-") or bo.color not in ("*", "O"):
                raise ValueError(f"GGF: BO[{value}] is not an 8x8 board of '*', 'O', '-' with '*' or 'O' to move")
        elif name in ("B", "W"):
            pos = value.split("/")[0].strip()
            if not (pos[:2].lower() == "pa" or _SQUARE.match(pos.lower())):
                raise ValueError(f"GGF: {name}[{value}] names no square")
            moves.append(MOVE(name, pos))
    if bo is None:
        raise ValueError("GGF: no BO[...] property")
    return GGF(bo, moves)


def parse_ggf_board_to_bitboard(squares):
    """(black, white) of BO's 64 squares: square i of the text is bit i (lib/util.py:20-27 of the reference reads them so)."""
    black = sum(1 << i for i, ch in enumerate(squares) if ch == "*")
    white = sum(1 << i for i, ch in enumerate(squares) if ch == "O")
    return black, white


def convert_to_bitboard_and_actions(ggf):
    """(black, white, actions) - actions in play order, None for a pass - of a parsed game."""
    black, white = parse_ggf_board_to_bitboard(ggf.BO.square_cont)
    return black, white, [convert_move_to_action(m.pos) for m in ggf.MOVES]
