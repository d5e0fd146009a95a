"""CPU: reading a game back from GGF text (lib/ggf.py parse_ggf, convert_to_bitboard_and_actions) - what the NBoard engine's
`set game` and lib/analysis.GameAnalyzer are fed with."""
import pytest

from reversi_alpha_zero_amd.lib.ggf import (convert_action_to_move, convert_move_to_action, convert_to_bitboard_and_actions, make_ggf_string,
                                            parse_ggf)

INIT_BLACK, INIT_WHITE = 0x0000000810000000, 0x0000001008000000


def test_initial_board_and_moves_of_a_written_game():
    text = make_ggf_string("b", "w", moves=["F5", "D6", "C3"], result="?")
    ggf = parse_ggf(text)
    assert ggf.BO.board_type == "8" and ggf.BO.color == "*" and len(ggf.BO.square_cont) == 64
    assert [(m.color, m.pos) for m in ggf.MOVES] == [("B", "F5"), ("W", "D6"), ("B", "C3")]
    assert convert_to_bitboard_and_actions(ggf) == (INIT_BLACK, INIT_WHITE, [44, 29, 18])


def test_other_board_with_white_to_move():
    squares = ["-"] * 64
    black, white = [0, 9, 63], [1, 62, 36]
    for i in black:
        squares[i] = "*"
    for i in white:
        squares[i] = "O"
    ggf = parse_ggf("(;GM[Othello]BO[8 %s O]W[A3];)" % "".join(squares))
    b, w, actions = convert_to_bitboard_and_actions(ggf)
    assert ggf.BO.color == "O" and b == sum(1 << i for i in black) and w == sum(1 << i for i in white) and actions == [2]


def test_tag_case_pass_entries_and_annotated_moves():
    board = "---------------------------O*------*O---------------------------"
    ggf = parse_ggf(f"(;gm[Othello]bo[8 {board} *]b[f5]w[D6//0.5]B[pa]w[PASS]B[c3/-1.25/3.2];)")
    assert [m.color for m in ggf.MOVES] == ["B", "W", "B", "W", "B"]
    assert convert_to_bitboard_and_actions(ggf)[2] == [44, 29, None, None, 18]


def test_move_naming_corners():
    for move, action in (("A1", 0), ("H8", 63), ("F5", 44), ("A8", 7), ("H1", 56)):
        assert convert_move_to_action(move) == action and convert_move_to_action(move.lower()) == action
        assert convert_action_to_move(action) == move
    assert convert_move_to_action("PA") is None and convert_move_to_action("pass") is None and convert_action_to_move(None) == "PA"


@pytest.mark.parametrize("text", [
    "(;GM[Othello]B[F5];)",                                                                       # no board
    "(;BO[8 ---------------------------O*------*O--------------------------- ];)",                # no side to move
    "(;BO[8 ---------------------------O*------*O-------------------------- *];)",                # 63 squares
    "(;BO[8 ---------------------------Ox------*O--------------------------- *];)",               # an unknown square
    "(;BO[10 ---------------------------O*------*O--------------------------- *];)",              # not 8x8
    "(;BO[8 ---------------------------O*------*O--------------------------- B];)",               # an unknown colour
    "(;BO[8 ---------------------------O*------*O--------------------------- *]B[I5];)",          # a file off the board
    "(;BO[8 ---------------------------O*------*O--------------------------- *]W[F9];)",          # a rank off the board
    "(;BO[8 ---------------------------O*------*O--------------------------- *]B[];)",            # no square at all
])
def test_malformed_input_raises(text):
    with pytest.raises(ValueError, match="GGF"):
        parse_ggf(text)
