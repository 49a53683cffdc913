"""CPU: the alignment grid's generator (tests/pkt_grid.py) -- every grid the GPU tests run is complete (the generator asserts every required cell itself), deterministic,
and its helpers name the right packet."""
import pkt_grid as PG


def test_every_grid_is_complete_and_deterministic():
    for G in (0, 4, 8, 16, 64):
        a, b = PG.Packed(G), PG.Packed(G)                       # (construction runs the completeness assertions)
        assert a.lens == b.lens and a.n > 16 * len(PG.all_lengths()) and all(0 <= l <= max(PG.all_lengths()) for l in a.lens)
        assert a.size == 2 * PG.GUARD + sum(a.lens)
    for G in (0, 4, 8, 16):
        s = PG.Scattered(G)
        assert s.n == 256 * len(PG.compact_lengths(G)) and s.pos_in == PG.Scattered(G).pos_in
    s = PG.Scattered(0, inplace=True)
    assert s.n == 16 * len(PG.all_lengths()) and s.pos_out is s.pos_in


def test_lengths_cover_the_loop_and_group_edges():
    full, lc = PG.all_lengths(), PG.compact_lengths()
    assert full[:273] == list(range(273)) and {16 * 129 + 1, 16 * 63 - 1, 16 * 33 + 1} <= set(full)
    assert {0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 271, 272} <= set(lc) and 34 <= len(lc) <= 45
    assert set(PG.group_edges(16)) <= set(PG.compact_lengths(16))
    assert PG.forged(15) == [0, 7, 14] and PG.forged(16) == [0, 7, 14, 15]


def test_a_difference_is_attributed_to_its_packet_or_guard():
    starts, lens = [256, 256, 260, 270], [0, 4, 3, 5]
    assert PG.owner(starts, lens, 257) == (1, 1) and PG.owner(starts, lens, 262) == (2, 2)
    assert PG.owner(starts, lens, 255) == (0, None) and PG.owner(starts, lens, 263) == (3, None) and PG.owner(starts, lens, 275) == (4, None)
    assert PG.first_difference(b"abcd", b"abcd") is None and PG.first_difference(b"abcd", b"abXd") == 2
