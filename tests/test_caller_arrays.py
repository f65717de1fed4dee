"""The arena of tests/caller_arrays.py on the CPU: where the placements put the arrays, and that check() names what changed and where."""
import numpy as np
import pytest
import torch

from tests.caller_arrays import GUARD, PLACEMENTS, SENTINEL, SENTINEL_BITS, Arena, ArenaError

# odd and even lengths; 585 = 13 * 9 * 5 is the x-face count of a 12 x 9 x 5 grid
SPEC = [("x", 585, "in"), ("y", 540, "inout"), ("z", 7, "out"), ("w", 6, "in"), ("u", 105, "in")]


def make(placement, spec=SPEC, **kw):
    a = Arena(spec, placement, "cpu", **kw)
    rng = np.random.default_rng(1)
    for n, l, r in spec:
        if r != "out":
            a.fill(n, rng.uniform(-1.0, 1.0, l))
    return a.freeze()


def test_sentinel_is_a_finite_number_of_order_one_with_its_own_bits():
    assert 1.0 < SENTINEL < 2.0 and np.float64(SENTINEL).view(np.int64) == SENTINEL_BITS
    assert np.float64(SENTINEL + 1e-3).view(np.int64) != SENTINEL_BITS            # a stray `+= x` shows


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_phases_offsets_and_guards(placement):
    a = make(placement)
    base = a.buf.data_ptr()
    assert base % 16 == 0
    want = {"A": [0, 0, 0, 0, 0], "B": [8, 8, 8, 8, 8], "C": [0, 8, 0, 8, 0], "D": [8, 0, 0, 8, 8]}[placement]
    assert [a.phase(n) for n, _, _ in SPEC] == want
    assert a.phases() == dict(zip(a.names, want))
    w = a.buf.numpy()
    end = 0
    for i, (n, l, r) in enumerate(SPEC):
        s = (a[n].data_ptr() - base) // 8
        assert s == a.start[n] and a[n].numel() == l and a[n].is_contiguous()
        gap = s - end
        if placement == "D":
            assert gap == (GUARD + 1 if i == 0 else 0)
        else:
            assert GUARD <= gap <= GUARD + 1
        # the guard in front: the sentinel beside an array that is written, NaN between inputs
        roles = {r} | ({SPEC[i - 1][2]} if i else set())
        if roles == {"in"}:
            assert np.isnan(w[end:s]).all()
        else:
            assert (w[end:s].view(np.int64) == SENTINEL_BITS).all()
        if r == "out":
            assert (w[s:s + l].view(np.int64) == SENTINEL_BITS).all()
        end = s + l
    assert a.total - end == GUARD and np.isnan(w[end:]).all()                         # the last array is an input
    a.check()


def test_an_odd_length_flips_the_phase_of_what_stands_behind_it_in_D():
    even = Arena([("a", 6, "in"), ("b", 4, "in"), ("c", 4, "in")], "D", "cpu")
    assert [even.phase(n) for n in "abc"] == [8, 8, 8]
    odd = Arena([("a", 6, "in"), ("b", 5, "in"), ("c", 4, "in"), ("d", 3, "in"), ("e", 2, "in")], "D", "cpu")
    assert [odd.phase(n) for n in "abcde"] == [8, 8, 0, 0, 8]
    # packed [Vx | Vy | Vz] of a 12 x 9 x 5 grid that is not periodic: 585 x-faces shift Vy and Vz by themselves
    faces = Arena([("Vx", 13 * 9 * 5, "inout"), ("Vy", 12 * 10 * 5, "inout"), ("Vz", 12 * 9 * 6, "inout")], "D", "cpu")
    assert [faces.phase(n) for n in ("Vx", "Vy", "Vz")] == [8, 0, 0]
    assert faces["Vy"].data_ptr() == faces["Vx"].data_ptr() + 8 * 585


def test_flip_moves_one_array_only():
    a = Arena(SPEC, "A", "cpu", flip=("y",))
    assert [a.phase(n) for n, _, _ in SPEC] == [0, 8, 0, 0, 0]
    b = Arena(SPEC, "B", "cpu", flip=("x", "u"))
    assert [b.phase(n) for n, _, _ in SPEC] == [0, 8, 8, 8, 0]


def raised(a, **kw):
    with pytest.raises(ArenaError) as e:
        a.check(**kw)
    return e.value


@pytest.mark.parametrize("placement", ["A", "B", "C"])
def test_a_stray_write_into_a_guard_is_named(placement):
    a = make(placement)
    a["z"][:] = 2.0
    a.check(written=["z"])
    a.buf[a.start["z"] + 7] = 0.5                    # one past the end of z
    e = raised(a, written=["z"])
    assert (e.array, e.where, e.offset) == ("z", "after", 1) and "'z'" in str(e) and "past the end" in str(e)
    a = make(placement)
    a.buf[a.start["y"] - 2] += 1.0                   # a read-modify-write two before y: the sentinel is not absorbing
    e = raised(a, written=["y"])
    assert (e.array, e.where, e.offset) == ("y", "before", 2) and "before the start" in str(e)
    a = make(placement)
    a.buf[a.start["x"] + 585 + 2] = 0.0              # a NaN guard between inputs turned into a number
    e = raised(a)
    assert (e.array, e.where, e.offset) == ("x", "after", 3)
    a = make(placement)
    a.buf[0] = 1.0                                   # the first word of the arena
    e = raised(a)
    assert (e.array, e.where, e.offset) == ("x", "before", a.start["x"])


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_a_write_into_an_input_or_an_unnamed_array_is_named(placement):
    a = make(placement)
    a["w"][3] = 9.0
    e = raised(a, written=["y", "z"])
    assert (e.array, e.where, e.offset) == ("w", "inside", 3) and "'w'" in str(e) and "(in," in str(e)
    a = make(placement)
    a["y"][11] = 9.0                                 # an inout array the call was not to write
    e = raised(a, written=["z"])
    assert (e.array, e.where, e.offset) == ("y", "inside", 11)
    a.check(written=["y", "z"], partial=["z"])       # named: allowed
    with pytest.raises(AssertionError):
        a.check(written=["x"])                       # an input can not be named


def test_a_write_into_the_first_word_of_a_packed_neighbour_is_named():
    a = make("D")
    a["x"][:] = a["x"] * 1.0
    assert a["y"].data_ptr() == a["x"].data_ptr() + 8 * 585
    a.buf[a.start["x"] + 585] = 0.25                 # one past the end of x is word 0 of y
    e = raised(a, written=["z"])
    assert (e.array, e.where, e.offset) == ("y", "inside", 0) and "behind the end of 'x'" in str(e)
    a = make("D")
    a.buf[a.start["z"] + 7] = 0.25                   # one past the end of the output z is word 0 of the input w
    e = raised(a, written=["z"], partial=["z"])
    assert (e.array, e.where, e.offset) == ("w", "inside", 0) and "behind the end of 'z'" in str(e)


def test_an_output_that_keeps_a_sentinel_is_named():
    a = make("B")
    a["z"][:5] = 3.0
    e = raised(a, written=["z"])
    assert (e.array, e.where, e.offset) == ("z", "inside", 5) and "still holds the sentinel" in str(e)
    a.check(written=["z"], partial=["z"])
    a["z"][5:] = 3.0
    a.check(written=["z"])


@pytest.mark.parametrize("placement", ["A", "B", "C"])
def test_a_read_past_an_input_shows_in_the_result(placement):
    """between inputs the guards are NaN: a sum that runs one word too far, on either side, is not finite"""
    a = make(placement)
    s, l = a.start["w"], 6
    assert np.isfinite(float(a.buf[s:s + l].sum()))
    assert not np.isfinite(float(a.buf[s:s + l + 1].sum()))
    assert not np.isfinite(float(a.buf[a.start["u"] - 1:a.start["u"] + 105].sum()))
    a["z"][0] = a.buf[a.start["u"]:a.start["u"] + 106].sum()          # ... and reaches an output
    a["z"][1:] = 0.0
    a.check(written=["z"])
    assert not np.isfinite(a.get("z")).all()
    # beside an array that is written the guard is the sentinel: a read-through there is a finite, wrong number (the reference comparison's part)
    assert float(a.buf[a.start["y"] - 1]) == SENTINEL


def test_fill_refuses_outputs_and_wrong_lengths():
    a = Arena(SPEC, "A", "cpu")
    with pytest.raises(AssertionError):
        a.fill("z", np.zeros(7))
    with pytest.raises(AssertionError):
        a.fill("x", np.zeros(584))
    with pytest.raises(AssertionError):
        a.check()                                     # not frozen
    assert torch.equal(a.fill("w", np.arange(6.0)), torch.arange(6.0, dtype=torch.float64))
