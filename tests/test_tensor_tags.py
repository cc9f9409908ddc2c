"""The by-products that one autograd node leaves on a tensor for the next (mulan_amd.ops._leave / _left / _carry,
DESIGN.md section 2): host logic on plain CPU tensors, no GPU and no library needed."""
import pytest
import torch

from mulan_amd import ops

TAGS = ("_absmax", "_gnstats", "_colsum", "_colsum_parts", "_bias_sink", "_bias_twin", "_biasdone", "_biasgrad", "_planes",
        "_grad_planes", "_accepts_grad_planes")


def test_a_tag_is_found_again_with_the_arity_it_was_left_with():
    t = torch.zeros(2, 8, 4)
    a, b = torch.ones(2, 16), torch.ones(3)
    assert ops._leave(t, "_absmax", a) is t
    assert ops._left(t, "_absmax") is a                         # one payload: the bare value
    ops._leave(t, "_planes", a, b)
    got = ops._left(t, "_planes")
    assert isinstance(got, tuple) and len(got) == 2 and got[0] is a and got[1] is b
    ops._leave(t, "_biasgrad", b, None)                         # a pair whose second member is None is still a pair
    assert ops._left(t, "_biasgrad")[0] is b and ops._left(t, "_biasgrad")[1] is None
    assert ops._left(t, "_accepts_grad_planes") is None
    ops._leave(t, "_accepts_grad_planes")
    assert ops._left(t, "_accepts_grad_planes") is True        # no payload: present, and truthy
    assert ops._left(t, "_gnstats") is None                     # never left
    assert ops._left(None, "_absmax") is None


def test_stored_layout_is_payload_first_and_stamp_last():
    t = torch.zeros(2, 8, 4)
    a, b = torch.ones(2, 16), torch.ones(3)
    ops._leave(t, "_absmax", a)
    ops._leave(t, "_biasdone", a, b)
    ops._leave(t, "_accepts_grad_planes")
    m, ver = t._absmax                                          # (the layout the GPU tests read)
    assert m is a and ver == t._version
    assert t._biasdone[0] is a and t._biasdone[1] is b and t._biasdone[-1] == t._version and len(t._biasdone) == 3
    assert t._accepts_grad_planes == (t._version,)


@pytest.mark.parametrize("tag", TAGS)
def test_an_in_place_write_invalidates_every_tag(tag):
    t = torch.zeros(2, 8, 4)
    payload = {"_accepts_grad_planes": (), "_absmax": (torch.ones(2, 16),)}.get(tag, (torch.ones(2, 4), torch.ones(4)))
    ops._leave(t, tag, *payload)
    assert ops._left(t, tag) is not None
    t.add_(1)
    assert ops._left(t, tag) is None
    ops._leave(t, tag, *payload)                                # left again for the new content: valid again
    assert ops._left(t, tag) is not None


def test_carry_keeps_the_view_tags_and_nothing_else():
    t = torch.zeros(2, 8, 4)
    m, st, cs = torch.ones(2, 16), torch.ones(2, 4, 1, 2), torch.ones(2, 4)
    for tag in TAGS:
        ops._leave(t, tag, *{"_absmax": (m,), "_gnstats": (st,), "_accepts_grad_planes": ()}.get(tag, (cs, cs)))
    v = ops._carry(t, t.view(2, 32))
    assert v.shape == (2, 32) and ops._left(v, "_absmax") is m and ops._left(v, "_gnstats") is st
    assert all(ops._left(v, tag) is None for tag in TAGS if tag not in ("_absmax", "_gnstats"))
    only = ops._carry(t, t.view_as(t), tags=("_absmax",))       # a site that keeps a smaller set says so
    assert ops._left(only, "_absmax") is m and ops._left(only, "_gnstats") is None
    pair = ops._carry(t, t.view_as(t), tags=("_planes",))       # several payloads travel as they were left
    assert ops._left(pair, "_planes")[0] is cs and len(pair._planes) == 3
    t.add_(1)                                                   # the view shares the version counter of its base
    assert ops._left(v, "_absmax") is None
    stale = ops._carry(t, t.view(2, 32))                        # nothing valid on the source: nothing to carry
    assert not hasattr(stale, "_absmax") and not hasattr(stale, "_gnstats")
    assert ops._carry(None, t.view(2, 32)).shape == (2, 32)


def test_carry_refuses_maxima_when_dim_0_changes():
    t = torch.zeros(2, 8, 4)
    m, st = torch.ones(2, 16), torch.ones(2, 4, 1, 2)
    ops._leave(t, "_absmax", m)
    ops._leave(t, "_gnstats", st)
    v = ops._carry(t, t.view(16, 4))
    assert ops._left(v, "_absmax") is None                      # one row of maxima per image: 2 rows do not describe 16
    assert ops._left(ops._carry(t, t.view(2, 32)), "_absmax") is m
    kept = ops.view_keep_absmax(t, 2, -1)
    assert kept.shape == (2, 32) and ops._left(kept, "_absmax") is m and ops._left(kept, "_gnstats") is None
    assert ops._left(ops.view_keep_absmax(t, -1, 4), "_absmax") is None


def test_leave_on_an_object_that_refuses_attributes_does_not_raise():
    class Sealed:
        __slots__ = ("_version",)

        def __init__(self):
            self._version = 0

    s = Sealed()
    assert ops._leave(s, "_absmax", torch.ones(2, 16)) is s
    assert ops._left(s, "_absmax") is None
    o = object()                                                # not even a version to stamp with
    assert ops._leave(o, "_absmax", 1) is o


def test_planes_only_stand_in_carries_its_planes_on_the_same_object(monkeypatch):
    monkeypatch.setattr(ops, "_NAN", {})
    planes, bound = torch.zeros(64, dtype=torch.uint8), torch.zeros(2, 16, dtype=torch.int32)
    g = ops._planes_only_grad((2, 8, 4), torch.device("cpu"), planes, bound)
    assert g.shape == (2, 8, 4) and bool(torch.isnan(g).all()) and all(s == 0 for s in g.stride())
    got = ops._left(g, "_grad_planes")
    assert got is not None and got[0] is planes and got[1] is bound
    assert ops._left(g, "_grad_planes")[0] is planes            # found again, on the same object
    other = ops._planes_only_grad((2, 8, 4), torch.device("cpu"), bound, planes)
    assert ops._left(other, "_grad_planes")[0] is bound and ops._left(g, "_grad_planes")[0] is planes
    assert ops._left(g.view_as(g), "_grad_planes") is None     # another tensor object over the stand-in: no planes
