"""CPU self-test of tests/guarded.py: the word comparison behind Guarded.check() / count_unwritten() on blocks as check() would
download them - one guard word flipped in front, one behind, one payload word never written - and the layout rules (guard size,
alignment, the alternation of the input pattern)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guarded as G      # noqa: E402

SHAPE = (3, 2, 1280)      # three packets of Nt = 4, Nr = 2


def _written_block(fill):
    g, n = G.guard_words(SHAPE), int(np.prod(SHAPE))
    rng = np.random.default_rng(1)
    data = rng.standard_normal(n).astype(np.float32)
    return g, n, data, G.make_block(g, n, fill, data)


def test_guard_size_and_alignment():
    assert G.guard_words(SHAPE) * 4 == 64 << 10                         # one packet (10 KiB) is below the 64-KiB floor
    big = (2, 4, 32, 234)                                                # one packet: 119 808 bytes = 468 x 256
    assert G.guard_words(big) * 4 == 119808
    assert G.guard_words((5, 234)) * 4 == 64 << 10
    odd = (2, 3, 9001)                                                   # 108 012 bytes: rounded up to the next 256
    assert G.guard_words(odd) * 4 == 108032 and G.guard_words(odd) * 4 % 256 == 0
    assert G.guard_words((7,)) * 4 == 64 << 10                           # a vector: the packet is one float


@pytest.mark.parametrize('start', range(8))
def test_every_16_byte_read_of_an_input_guard_meets_nan_and_both_signs(start):
    g = G.guard_pattern(64, 'in').view(np.float32)
    quad = g[start:start + 4]
    assert np.isnan(quad).sum() == 2 and (quad == np.float32(3.0e38)).sum() == 1 and (quad == np.float32(-3.0e38)).sum() == 1
    # what the two kinds of silent consumer make of it: a NaN-ignoring maximum sees 3e38, a product with a zero weight sees NaN
    assert np.fmax.reduce(np.abs(quad)) == np.float32(3.0e38)
    assert np.isnan((quad * np.float32(0.0)).sum())
    out = G.guard_pattern(64, 'out')
    assert (out[0::2] == G.GUARD_NAN).all() and (out[1::2] == G.GUARD_ONE).all()
    assert np.isnan(out.view(np.float32)[0::2]).all() and (out.view(np.float32)[1::2] + np.float32(1e-6) != out.view(np.float32)[1::2]).all()
    # three NaNs of different payload: a NaN handed on from an input guard is visible in an output guard and in an output's payload
    nans = np.array([G.GUARD_NAN, G.INPUT_NAN, G.UNWRITTEN], np.uint32)
    assert len(set(nans.tolist())) == 3 and np.isnan(nans.view(np.float32)).all() and ((nans >> 22) & 1).all(), 'quiet NaNs'
    assert (G.guard_pattern(64, 'in')[0::2] == G.INPUT_NAN).all()


@pytest.mark.parametrize('fill', ['in', 'out'])
def test_an_untouched_block_passes(fill):
    g, n, data, block = _written_block(fill)
    rep = G.check_block(block, g, n, fill)
    assert rep['front'] is None and rep['back'] is None and rep['unwritten'].size == 0
    assert np.array_equal(block[g:g + n].view(np.float32), data)
    fresh = G.make_block(g, n, fill)                                      # before the call: the whole payload is unwritten
    assert G.inspect_block(fresh, g, n, fill)['unwritten'].size == n and G.check_block(fresh, g, n, fill)['front'] is None


@pytest.mark.parametrize('fill', ['in', 'out'])
def test_each_injected_defect_is_reported_with_its_offset(fill):
    g, n, data, clean = _written_block(fill)
    front, back, hole = g - 3, g + n + 5, 777
    # one at a time: each defect alone must be seen
    b = clean.copy()
    b[front] ^= 1
    rep = G.inspect_block(b, g, n, fill)
    assert rep['front'] == (front, 3, 1) and rep['front_nearest'] == (front, 3, 1) and rep['back'] is None and rep['unwritten'].size == 0
    with pytest.raises(G.GuardDamage) as err:
        G.check_block(b, g, n, fill, 'plane')
    assert 'plane front guard' in str(err.value) and 'offset %d' % front in str(err.value) and '12 bytes' in str(err.value)
    b = clean.copy()
    b[back] = np.float32(0.0).view(np.uint32)
    rep = G.inspect_block(b, g, n, fill)
    assert rep['back'] == (back, 6, 1) and rep['front'] is None and rep['unwritten'].size == 0
    with pytest.raises(G.GuardDamage) as err:
        G.check_block(b, g, n, fill, 'plane')
    assert 'plane back guard' in str(err.value) and 'offset %d' % back in str(err.value) and 'byte 20 past' in str(err.value)
    b = clean.copy()
    b[g + hole] = G.UNWRITTEN
    rep = G.check_block(b, g, n, fill)                                    # guards intact: no exception, the hole is counted
    assert rep['front'] is None and rep['back'] is None and rep['unwritten'].tolist() == [hole]
    # all three in one block, as a broken kernel would leave it
    b = clean.copy()
    b[front] ^= 1
    b[back] = 0
    b[g + hole] = G.UNWRITTEN
    rep = G.inspect_block(b, g, n, fill)
    assert rep['front'][:2] == (front, 3) and rep['back'][:2] == (back, 6) and rep['unwritten'].tolist() == [hole]
    with pytest.raises(G.GuardDamage) as err:
        G.check_block(b, g, n, fill)
    assert 'front guard' in str(err.value) and 'back guard' in str(err.value)


def test_first_and_nearest_damage_and_the_edges():
    g, n, data, clean = _written_block('out')
    b = clean.copy()
    b[[0, 10, g - 1]] = 0                                                  # first word of the block ... the word that touches the payload
    b[[g + n, 2 * g + n - 1]] = 0                                          # the word behind the payload ... the last of the block
    rep = G.inspect_block(b, g, n, 'out')
    assert rep['front'] == (0, g, 3) and rep['front_nearest'] == (g - 1, 1, 3)
    assert rep['back'] == (g + n, 1, 2)
    # a guard word overwritten with the OTHER word of the input pattern is damage too (a shifted copy of the guard)
    b = G.make_block(g, n, 'in', data)
    b[g + n + 1] = G.INPUT_NAN
    assert G.inspect_block(b, g, n, 'in')['back'] == (g + n + 1, 2, 1)
    # ... and so is the NaN of an input guard in an output guard: what a kernel stores that computed on words it read out of bounds
    b = G.make_block(g, n, 'out', data)
    b[g + n] = G.INPUT_NAN
    assert G.inspect_block(b, g, n, 'out')['back'] == (g + n, 1, 1)
