"""Shared by the replay-buffer tests: tuples (codes, pi, z) from short random legal games on alphapig_amd.game.Board, so
that all four stone ages and both colours occur in the codes."""
import numpy as np

from alphapig_amd.game import Board


def random_game_tuples(width, n_in_row, n_tuples, seed):
    """-> (codes u8 [n][stride], pis f32 [n][HW], zs f32 [n]): the position before every ply of random games of 3 to 24
    plies (alternating start player), a random normalised pi and z = +-1."""
    rs = np.random.RandomState(seed)
    hw = width * width
    codes = []
    game = 0
    while len(codes) < n_tuples:
        b = Board(width=width, height=width, n_in_row=n_in_row)
        b.init_board(game % 2)
        game += 1
        for m in rs.permutation(hw)[:rs.randint(3, 25)]:
            codes.append(b.position_codes())
            b.do_move(int(m))
    codes = np.stack(codes[:n_tuples])
    pis = rs.rand(n_tuples, hw).astype(np.float32)
    pis /= pis.sum(axis=1, keepdims=True)
    zs = rs.choice(np.array([-1.0, 1.0], np.float32), n_tuples)
    return codes, pis, zs


def episodes(width, n_in_row, n_extends, seed, lo=1, hi=40):
    """n_extends blocks of lo ... hi tuples, as successive extend calls deliver them"""
    rs = np.random.RandomState(seed + 1000)
    sizes = [int(rs.randint(lo, hi + 1)) for _ in range(n_extends)]
    codes, pis, zs = random_game_tuples(width, n_in_row, sum(sizes), seed)
    out, at = [], 0
    for s in sizes:
        out.append((codes[at:at + s], pis[at:at + s], zs[at:at + s]))
        at += s
    return out
