"""The per-step hand-offs between layers (ops._SLOTS): named records in one mailbox (ops._park / ops._take), the
ResGradHolder methods, and ops.reset_step_state, which has to know every slot.  Host-side logic only: no kernel runs."""
import pytest
import torch

import convnet_amd as ca

ops = ca.ops
Err = ca._lib.ConvNetHipError


def _records(t):
    return {'_lazy_z': ops.LazyZ(t, t, t, None, t, None, True), '_lazy_a': ops.LazyA(t, t, t, True),
            '_lazy_dy': ops.LazyDy(t, t, t), '_bwd_partials': ops.BwdPartials(t, 3), '_deferred': ops.DeferredBN(t),
            '_q_stash': ops.QStash(8, t, t)}


def test_every_slot_has_a_record_here():
    assert set(_records(torch.zeros(1))) == set(ops._SLOTS)


def test_reset_step_state_empties_every_slot():
    """Before the slots were one list, reset_step_state left _bwd_partials, _deferred and _q_stash behind; a stale
    _bwd_partials is matched by address and shape only, which the caching allocator hands out again after an aborted step."""
    t = torch.zeros(2, 3)
    child, holder_owner = torch.nn.Module(), torch.nn.Module()
    model = torch.nn.Sequential(torch.nn.Sequential(child), holder_owner)
    for slot, rec in _records(t).items():
        ops._park(child, slot, t, rec)
    child._fwd_ctx = lambda: None
    holder_owner._res_holder = ops.ResGradHolder()
    holder_owner._res_holder.park(t, 2)
    assert all(slot in child.__dict__ for slot in ops._SLOTS) and '_q_stash' in child.__dict__
    ops.reset_step_state(model)
    for slot in ops._SLOTS + ('_q_stash', '_fwd_ctx'):
        assert child.__dict__.get(slot) is None, slot
        assert ops._take(child, slot) is None, slot
    assert holder_owner._res_holder.take() == (None, 1, False)


@pytest.mark.parametrize('slot', ops._SLOTS)
def test_take_is_one_shot(slot):
    t = torch.zeros(2, 3)
    mod = torch.nn.Module()
    rec = _records(t)[slot]
    ops._park(mod, slot, t, rec)
    assert ops._take(mod, slot, t) is rec
    assert ops._take(mod, slot, t) is None
    ops._park(mod, slot, t, rec)      # (no owner given: taken unchecked)
    assert ops._take(mod, slot) is rec and ops._take(mod, slot) is None


def test_park_refuses_an_unknown_slot():
    mod = torch.nn.Module()
    with pytest.raises(Err, match='unknown'):
        ops._park(mod, '_lazy_b', torch.zeros(1), ops.LazyDy(None, None, None))
    assert '_lazy_b' not in mod.__dict__


def _strangers(t):
    """An owner at another address, and one at t's address with another shape."""
    return {'address': torch.zeros_like(t), 'shape': t.view(-1)}


@pytest.mark.parametrize('other', ['address', 'shape'])
@pytest.mark.parametrize('slot,text', [('_lazy_z', "is not this convolution's input"),
                                       ('_lazy_a', "is not this convolution's input"),
                                       ('_lazy_dy', "does not belong to this convolution's output")])
def test_mismatch_raises_for_the_lazy_operands(slot, text, other):
    t = torch.zeros(2, 3)
    stranger = _strangers(t)[other]
    assert (stranger.data_ptr() == t.data_ptr()) == (other == 'shape')
    mod = torch.nn.Module()
    ops._park(mod, slot, t, _records(t)[slot])
    with pytest.raises(Err) as e:
        ops._take(mod, slot, stranger)
    assert text in str(e.value)
    # (the owner's key - what Conv2dFunction keeps of its output for the backward pass - serves as the owner)
    ops._park(mod, slot, t, _records(t)[slot])
    with pytest.raises(Err) as e:
        ops._take(mod, slot, ops._owner_key(stranger))
    assert text in str(e.value)
    ops._park(mod, slot, t, _records(t)[slot])
    assert ops._take(mod, slot, ops._owner_key(t)) == _records(t)[slot]


@pytest.mark.parametrize('other', ['address', 'shape'])
@pytest.mark.parametrize('slot', ['_bwd_partials', '_q_stash'])
def test_mismatch_means_not_fused_for_the_silent_slots(slot, other):
    t = torch.zeros(2, 3)
    mod = torch.nn.Module()
    ops._park(mod, slot, t, _records(t)[slot])
    assert ops._take(mod, slot, _strangers(t)[other], strict=False) is None
    assert slot not in mod.__dict__          # nothing left behind for a later tensor at that address
    assert ops._take(mod, slot, t, strict=False) is None


def test_deferred_mismatch_raises():
    t = torch.zeros(2, 3)
    mod = torch.nn.Module()
    ops._park(mod, '_deferred', t, ops.DeferredBN(t))
    with pytest.raises(Err, match='cannot apply it'):
        ops._take(mod, '_deferred', torch.zeros_like(t))


def test_refuse_parked_knows_every_slot():
    t = torch.zeros(2, 3)
    for slot, rec in _records(t).items():
        mod = torch.nn.Module()
        ops._refuse_parked(mod, 'grouped convolution')
        ops._park(mod, slot, t, rec)
        with pytest.raises(Err, match='grouped convolution'):
            ops._refuse_parked(mod, 'grouped convolution')


def test_records_are_plain_tuples():
    """tests/test_step_streaming_kernels_b256.py (GPU only) indexes and unpacks what conv2d_fwd_lazyz / conv2d_fwd_lazya
    are handed, and tests/test_ops.py / tests/test_exact.py hand them plain tuples."""
    assert ops.LazyZ._fields == ('y', 'residual', 'stats', 'res_stats', 'z', 'mask', 'relu')
    assert ops.LazyA._fields == ('bn_y', 'stats', 'a', 'relu')
    assert ops.LazyDy._fields == ('g', 'bn_y', 'coef')
    assert ops.BwdPartials._fields == ('partial', 'rows')
    assert ops.DeferredBN._fields == ('stats',)
    assert ops.BnBwdOperands._fields == ('y', 'mask', 'stats', 'relu')
    t = (1, 2, 3, None, 5, 6, True)
    lz = ops.LazyZ(*t)
    assert lz == t and isinstance(lz, tuple) and not hasattr(lz, '__dict__')
    assert lz[0] == 1 and lz[3] is None and lz.res_stats is None and lz[1:] == t[1:]
    y3, res, stats, res_stats, z, mask, relu = lz
    assert (y3, res, stats, res_stats, z, mask, relu) == t
    assert ops.LazyZ(*lz) == t      # normalising a record is the identity
    la = ops.LazyA(*(1, 2, 3, False))
    bn_y, stats, a, relu = la
    assert la == (1, 2, 3, False) and la[0] == 1 and (bn_y, stats, a, relu) == (1, 2, 3, False)
    with pytest.raises(TypeError):
        ops.LazyZ(*t[:6])


def test_res_grad_holder_park_take():
    h = ops.ResGradHolder()
    assert h.take() == (None, 1, False)
    t = torch.zeros(2)
    h.park(t)
    dres, sub, fused = h.take()
    assert dres is t and sub == 1 and fused is False
    assert h.take() == (None, 1, False)
    h.park(t, 2)
    assert h.take()[1] == 2 and h.dres is None and h.sub == 1
    h.park(t, 2)
    assert h.claim() == (t, 2)      # the second branch's dgrad adds it: the fork is told so
    assert h.take() == (t, 2, True) and h.take() == (None, 1, False)
    h.claim()
    h.park(t)                       # a new first gradient is not fused
    assert h.take() == (t, 1, False)
