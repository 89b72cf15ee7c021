"""GPU parity of Dht::searchStep on the resident searches (dhtgpu_srs_*, opendht_amd/csrc/srstep.hip)
against the model of srstep_cases.py.  Every comparison is exact: out_send and out4 of every step, and
rows, flags, lengths, status words, request states and ticks of every slot after every op of every
script.  Marked gpu: run on the MI355X box."""
import numpy as np
import pytest

import ncresolve_cases as NR
import oracle as O
import rsearch_cases as RS
import srstep_cases as SS
from srstep_cases import B_DONE, B_EXPIRED, B_OVER, B_REFILLED, B_SKIPPED, E, u32

pytestmark = pytest.mark.gpu

EINVAL, ENOIDS, ERANGE = -1, -4, -6


@pytest.fixture(scope="module")
def ctx():
    import opendht_amd
    c = opendht_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scripts():
    """every case, built once (and run on the model once: the scripts' own)"""
    return dict(SS.all_scripts())


def assert_state(ctx, model, what):
    for g, w, nm in zip(SS.ctx_state(ctx, len(model.slots)), SS.model_state(model), SS.STATE_NAMES):
        bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, f"{what}: {nm} of {bad.size} slots differ, first slot {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}"


def code(f, *a):
    import opendht_amd
    with pytest.raises(opendht_amd.DhtGpuError) as e:
        f(*a)
    return e.value.code


@pytest.mark.parametrize("name", [n for n, _ in SS.all_scripts()])
def test_scripts(ctx, scripts, name):
    """Every script on a context, compared with the model after every op; steps of 1, 4 and 5 searches
    (four waves per workgroup: 5 crosses a block), lists of up to 54 entries, up to 64 slots."""
    model = SS.Model()
    for k, step in enumerate(scripts[name].steps):
        want, got = SS.run_step(step, model, ctx)
        what = f"{name} step {k} {step[0]}"
        if step[0] in ("step", "offer"):
            for g, w, nm in zip(got, want, ("out_send", "out4") if step[0] == "step" else ("cnt", "touched", "stats")):
                assert np.array_equal(g, w), f"{what}: {nm} differ: got {g[(g != w).reshape(g.shape[0], -1).any(axis=1)][:3]} " \
                                             f"want {w[(g != w).reshape(w.shape[0], -1).any(axis=1)][:3]}"
        elif want is not None:
            assert np.array_equal(got, want), f"{what}: results differ"
        if model.slots and step[0] not in ("nc_set", "nc_accept", "clock"):
            assert_state(ctx, model, what)


def test_refill_leg_needs_a_mirror_only_when_asked():
    """refill_count 0 without an nc mirror is fine; 14 without one is DHTGPU_ENOIDS; with a small
    mirror the step's refill equals sr_refill followed by a step without one"""
    import opendht_amd
    keys = O.gen_ids(901, 200)
    targets = O.gen_ids(902, 5)
    slots = np.arange(5, dtype=np.uint32)
    with opendht_amd.Context(0) as a, opendht_amd.Context(0) as b:
        for c in (a, b):
            c.sr_reset(5)
            c.sr_open(slots, targets)
            c.srs_set_clock(1000)
        assert code(a.srs_step, slots, E, 14) == ENOIDS
        a.nc_set(keys)
        b.nc_set(keys)
        send_a, out_a = a.srs_step(slots, E, 14)
        assert (out_a[:, 2] == 14).all() and (out_a[:, 3] == B_REFILLED).all() and (out_a[:, :2] == 4).all()
        assert (b.sr_refill(slots, 14) == 14).all()
        send_b, out_b = b.srs_step(slots, E, 0)
        assert np.array_equal(send_a, send_b) and np.array_equal(out_a[:, :2], out_b[:, :2]) and not out_b[:, 2:].any()
        for x, y in zip(SS.ctx_state(a, 5), SS.ctx_state(b, 5)):
            assert np.array_equal(x, y)
    with opendht_amd.Context(0) as c:      # no mirror at all
        c.sr_reset(2)
        c.sr_open(slots[:2], targets[:2])
        c.srs_set_clock(1000)
        _, out4 = c.srs_step(slots[:2], E, 0)
        assert out4.tolist() == [[0, 0, 0, B_EXPIRED | B_DONE]] * 2     # an empty list expires


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(torch.device("cuda", 0))


def test_dev_forms_chained_on_one_stream():
    """ncr_find_dev -> sr_insert_dev with tokens -> srs_step_dev -> srs_entries_dev on a side stream,
    nothing from the host in between; slot list entries >= nslots are skipped and their output rows
    stay as they were"""
    import opendht_amd
    import torch
    dev = torch.device("cuda", 0)
    nkeys, nslots, per = 256, 6, 9
    keys = O.gen_ids(911, nkeys)
    handles = (np.random.default_rng(6).permutation(nkeys) + 50).astype(np.uint32)
    targets = O.gen_ids(912, nslots)
    slots = np.arange(nslots, dtype=np.uint32)
    pick = np.random.default_rng(7).choice(nkeys, size=nslots * per, replace=False)
    ids, hs = keys[pick], handles[pick]
    tok = (np.arange(nslots * per) % 3 != 0).astype(np.uint8)
    off = RS.csr(np.full(nslots, per))
    model = SS.Model()
    model.reset(nslots)
    model.open(slots, targets)
    model.set_clock(777)
    model.insert(slots, off, hs, ids, tok)
    want = model.step(slots, E, 0)
    call = np.array([0, 1, nslots, 2, 3, 0xFFFFFFF0, 4, 5], np.uint32)      # two entries name no slot
    real = [0, 1, 3, 4, 6, 7]
    with opendht_amd.Context(0) as c:
        c.nc_set(keys, handles)
        c.sr_reset(nslots)
        c.sr_open(slots, targets)
        c.srs_set_clock(777)
        tot, m = nslots * per, call.shape[0]
        stride = tot + 3
        d_p = _dev(NR.id_planes(ids, stride), np.int32)
        d_slots, d_call, d_off, d_tok = _dev(slots, np.int32), _dev(call, np.int32), _dev(off, np.int64), _dev(tok, np.uint8)
        d_h = torch.zeros(tot, dtype=torch.int32, device=dev)
        d_send = torch.full((m, 64), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        d_out4 = torch.full((m, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        d_req = torch.full((m, 64), 0x5A, dtype=torch.uint8, device=dev)
        d_tick = torch.full((m, 64), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        side = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        s = side.cuda_stream
        c.ncr_find_dev(d_p.data_ptr(), stride, tot, d_h.data_ptr(), None, s)
        c.sr_insert_dev(d_slots.data_ptr(), nslots, d_off.data_ptr(), d_h.data_ptr(), d_p.data_ptr(), stride,
                        d_tok.data_ptr(), None, s)
        c.srs_step_dev(d_call.data_ptr(), m, E, 0, d_send.data_ptr(), d_out4.data_ptr(), s)
        c.srs_entries_dev(d_call.data_ptr(), m, d_req.data_ptr(), d_tick.data_ptr(), s)
        side.synchronize()
        send, out4 = d_send.cpu().numpy().view(np.uint32), d_out4.cpu().numpy().view(np.uint32)
        req, tick = d_req.cpu().numpy(), d_tick.cpu().numpy().view(np.uint32)
        assert np.array_equal(send[real], want[0]) and np.array_equal(out4[real], want[1])
        wreq, wtick = model.entries(slots)
        assert np.array_equal(req[real], wreq) and np.array_equal(tick[real], wtick)
        assert wreq.any() and (wtick == 777).any()
        for j in (2, 5):
            assert (send[j] == 0x5A5A5A5A).all() and (out4[j] == 0x5A5A5A5A).all()
            assert (req[j] == 0x5A).all() and (tick[j] == 0x5A5A5A5A).all()
        for g, w, nm in zip(SS.ctx_state(c, nslots), SS.model_state(model), SS.STATE_NAMES):
            assert np.array_equal(g, w), nm


def test_argument_errors():
    """the clock unset, now = 0, val = 3, repeated slots, a slot >= nslots, ENOIDS before the first
    reset; a failed check changes nothing"""
    import opendht_amd
    ids = O.gen_ids(921, 4)
    slots = np.arange(3, dtype=np.uint32)
    with opendht_amd.Context(0) as c:
        for f, a in ((c.srs_step, (slots, E, 0)), (c.srs_entries, (slots,)), (c.srs_set_request, (slots, [1, 2, 3], 1))):
            assert code(f, *a) == ENOIDS, f.__name__
        assert code(c.srs_set_clock, 0) == ERANGE
        c.sr_reset(3)
        c.sr_open(slots, ids[:3])
        c.sr_insert(slots[:1], RS.csr([2]), u32([7, 8]), ids[2:4])
        assert code(c.srs_step, slots, E, 0) == EINVAL               # no clock yet
        assert code(c.srs_set_clock, 0) == ERANGE
        assert code(c.srs_step, slots, E, 0) == EINVAL               # still none
        c.srs_set_clock(5)
        assert code(c.srs_set_request, slots[:1], [7], 3) == EINVAL
        assert code(c.srs_set_request, [3], [7], 1) == EINVAL
        assert code(c.srs_step, [0, 1, 0], E, 0) == EINVAL
        assert code(c.srs_step, [0, 3], E, 0) == EINVAL
        assert code(c.srs_step, slots, E, 33) == EINVAL              # refill_count > DHTGPU_MAX_K
        assert code(c.srs_entries, [3]) == EINVAL
        req, tick = c.srs_entries(slots)
        assert not req.any() and not tick.any() and c.sr_status(slots)[:, 0].tolist() == [2, 0, 0]
        c.srs_set_request([0, 0], [7, 99], [2, 1])                   # 99 is in no list: nothing
        assert c.srs_entries(slots)[0][0, :3].tolist() == [2, 0, 0] or c.srs_entries(slots)[0][0, :3].tolist() == [0, 2, 0]
        send, out4 = c.srs_step(np.zeros(0, np.uint32), E, 0)        # m == 0: a no-op
        assert send.shape == (0, 64) and out4.shape == (0, 4)


def test_overflowing_refill_reports_erange_after_applying():
    """A list of 60 expired nodes behind 2 good ones; the step's refill brings 14 closer good nodes in:
    two fit, the row is full at 64, the others are dropped.  The host form raises DHTGPU_ERANGE with
    the results, bit1 is set and stays, and the sends went out."""
    import opendht_amd
    keys = O.gen_ids(931, 100)
    target = O.gen_ids(932, 1)
    far = 1 << 159
    good = keys[[(int.from_bytes(bytes(k), "big") ^ int.from_bytes(bytes(target[0]), "big")) < far for k in keys]]
    assert good.shape[0] >= 14
    bad_h = np.arange(1000, 1060, dtype=np.uint32)
    state = np.zeros(1100, np.uint8)
    state[bad_h] = 1
    with opendht_amd.Context(0) as c:
        c.nc_set(good, np.arange(good.shape[0], dtype=np.uint32) + 10)
        c.sr_reset(1)
        c.sr_set_state(state)
        c.sr_open([0], target)
        c.sr_insert([0], RS.csr([62]), np.concatenate([u32([5, 6]), bad_h]),
                    SS.ids_at(target[0], [far + 1, far + 2] + [far + 10 + i for i in range(60)]))
        assert c.sr_status([0])[0].tolist() == [62, 60, 0, 0]
        c.srs_set_clock(1000)
        with pytest.raises(opendht_amd.DhtGpuError) as e:
            c.srs_step([0], E, 14)
        assert e.value.code == ERANGE
        send, out4 = e.value.result
        assert out4[0].tolist() == [4, 4, 2, B_REFILLED | B_OVER]
        assert c.sr_status([0])[0].tolist() == [64, 60, 0, 2]
        assert send[0, :4].tolist() == c.sr_lists([0])[0][0, :4].tolist() and (send[0, 4:] == SS.NONE).all()
        assert c.srs_entries([0])[0][0, :5].tolist() == [1, 1, 1, 1, 0]
        _, out4 = c.srs_step([0], E, 14)                 # refill_tick is now: not due, nothing dropped
        assert out4[0].tolist() == [0, 4, 0, B_OVER]


def test_cpp_adapter_on_device(tmp_path):
    """tests/cpp/srstep_check.cpp --run --quick: ResidentSearches::noteRequest / stepBatch against the
    check's struct-based searchStep through seeded traffic"""
    import cpp_check
    cpp_check.run(cpp_check.build("srstep", tmp_path), ["--run", "--quick"], "srstep_check (device paths)", 120)
