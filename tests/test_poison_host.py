"""Tests of tests/poison.py itself, on CPU tensors: leaky fake operators are caught at the right rung of the ladder, a clean
one passes, the patch is undone on exit."""
import pytest
import torch

import poison


def test_patterns_are_what_the_docstring_says():
    with poison.poisoned("zeros") as p:
        a = torch.empty(5, dtype=torch.float32)
        b = torch.empty(3, dtype=torch.bool)
    assert not a.any() and not b.any() and p.count == 2 and p.bytes == 23
    with poison.poisoned("one") as p:
        i64, i32 = torch.empty(3, dtype=torch.int64), torch.empty(5, dtype=torch.int32)
        f, u8 = torch.empty(4, dtype=torch.float32), torch.empty(11, dtype=torch.uint8)
        b = torch.empty(3, dtype=torch.bool)
    assert i64.tolist() == [1, 1, 1] and i32.tolist() == [1, 0, 1, 0, 0]          # 20 bytes: two words, four trailing zeros
    assert f.view(torch.int32).tolist() == [1, 0, 1, 0] and float(f.abs().max()) < 1e-40
    assert u8.tolist() == [1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0] and b.view(torch.uint8).tolist() == [1, 1, 1]
    with poison.poisoned("nan") as p:
        f, d = torch.empty(2, 3), torch.empty(3, dtype=torch.float64)
        i, u = torch.empty(3, dtype=torch.int32), torch.empty(3, dtype=torch.uint8)
        b = torch.empty(2, dtype=torch.bool)
        like = torch.empty_like(f)
        new = f.new_empty(7)
        half = torch.empty(3, dtype=torch.float16)
        scalar = torch.empty((), dtype=torch.float32)
        nothing = torch.empty(0, 4)
    assert torch.isnan(f).all() and torch.isnan(d).all() and i.tolist() == [-1] * 3 and u.tolist() == [255] * 3
    assert b.view(torch.uint8).tolist() == [1, 1] and torch.isnan(like).all() and torch.isnan(new).all() and new.shape == (7,)
    assert torch.isnan(half).all() and torch.isnan(scalar) and nothing.numel() == 0
    assert p.count == 9 and p.bytes == 24 + 24 + 12 + 3 + 2 + 24 + 28 + 6 + 4      # the zero-size tensor is not counted


def test_the_slice_idiom_is_filled_behind_the_slice():
    with poison.poisoned("nan"):
        t = torch.empty(4, 8)[:, :5]
    assert torch.isnan(t).all() and t.shape == (4, 5)


def test_requires_grad_and_out_pass_through():
    with poison.poisoned("nan") as p:
        leaf = torch.empty(3, requires_grad=True)
        mine = torch.ones(3)
        torch.empty(3, out=mine)
    assert leaf.requires_grad and leaf.is_leaf and torch.isnan(leaf).all()
    assert mine.tolist() == [1.0, 1.0, 1.0] and p.count == 1


def test_attributes_are_restored_also_after_a_raise():
    before = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with pytest.raises(KeyError):
        with poison.poisoned("one"):
            assert torch.empty is not before[0] and torch.Tensor.new_empty is not before[2]
            raise KeyError("from inside")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before
    with pytest.raises(ValueError):
        with poison.poisoned("ones"):
            pass
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == before


def test_an_unwritten_output_element_is_caught_under_nan():
    seen = []

    def leaky():
        out = torch.empty(4)
        out[0], out[1], out[3] = 1.0, 2.0, 3.0
        seen.append(float(out[2]))
        return [out * 2.0 + 1.0]              # the denormal of `one` rounds away, as it would in any kernel's arithmetic

    with pytest.raises(AssertionError, match="under 'nan'"):
        poison.check(leaky, finite=False, unpatched=False)
    assert seen[:2] == [0.0, 1.4012984643248171e-45] and seen[2] != seen[2] and len(seen) == 3
    with pytest.raises(AssertionError):       # and with the finiteness check on as well
        poison.check(leaky, unpatched=False)


def test_an_unwritten_index_is_caught_under_one_and_nan_is_not_reached():
    table = torch.tensor([10.0, 20.0, 30.0])
    seen = []

    def leaky():
        idx = torch.empty(2, dtype=torch.int64)
        idx[0] = 2                             # idx[1] is never written, and read below
        seen.append(int(idx[1]))
        assert idx[1] >= 0, "the ladder handed a fake kernel an index of -1"
        return [table[idx]]

    with pytest.raises(AssertionError, match="under 'one'"):
        poison.check(leaky, unpatched=False)
    assert seen == [0, 1]


def test_an_operator_that_writes_everything_passes_and_the_counter_is_positive():
    def clean():
        x = torch.arange(6, dtype=torch.float32)
        out = torch.empty(6)
        scratch = torch.empty(6, dtype=torch.int32)
        scratch.copy_(torch.arange(6))
        out.copy_(x * 2 + scratch)
        return [out, scratch]

    rep = poison.check(clean)
    for pattern in poison.PATTERNS:
        assert rep[pattern].bytes == 48 and rep[pattern].count == 2
    assert rep["outputs"][0].tolist() == [0.0, 3.0, 6.0, 9.0, 12.0, 15.0]


def test_a_case_that_allocates_nothing_is_refused_as_vacuous():
    with pytest.raises(AssertionError, match="checks nothing"):
        poison.check(lambda: [torch.zeros(3)])


def test_bit_equality_sees_negative_zero_and_nan_payloads():
    assert not poison.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    a = torch.tensor([0x7FC00000, 0x7FC00001], dtype=torch.int32).view(torch.float32)
    assert poison.same_bits(a[:1], a[:1].clone()) and not poison.same_bits(a[:1], a[1:])
    assert poison.same_bits(torch.tensor([True, False]), torch.tensor([True, False]))
    assert not poison.same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.int32))
