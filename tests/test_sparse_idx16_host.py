"""``SparseState.index_wire`` on the CPU: the format's size, the four C entries' refusals (which
precede any device call), the option's parsing and refusals, and the bit formula.

(The kernels and the hooks on a GPU: tests/test_gpu_sparse_idx16.py.)"""
import ctypes
import os

import pytest
import torch

import sparse_idx16_format as F
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket
from allreducetopk_amd.build import LIB, build
from allreducetopk_amd.comm_hooks import sparse_hook as SH
from allreducetopk_amd.comm_hooks import sparse_hook_c4 as SH4

a = N.i64_array
NAMES = ("arctopk_sparse_idx16_bytes", "arctopk_sparse_idx16_pack", "arctopk_sparse_idx16_unpack",
         "arctopk_sparse_decode_idx16")


@pytest.fixture(scope="module")
def entries():
    if not os.path.exists(LIB):
        build()
    L = ctypes.CDLL(LIB)
    fns = {}
    for name in NAMES:
        fns[name] = getattr(L, name)
        fns[name].restype, fns[name].argtypes = N._SIGS[name]
    return fns


@pytest.mark.parametrize("numels,ks", [([1], [1]), ([65535, 65536, 65537, 131073], [7, 8, 9, 65537]),
                                       ([5, 1024, 7], [1, 256, 1]), ([33] * 70, [8] * 70), ([2 ** 31 - 1], [3])])
def test_bytes(entries, numels, ks):
    offs = [sum(numels[:i]) for i in range(len(numels))]
    koff = [sum(ks[:i]) for i in range(len(ks))]
    got = entries[NAMES[0]](sum(numels), len(numels), a(offs), a(ks), a(koff))
    assert got == F.wire_bytes(numels, ks) and got % 16 == 0


def test_refusals_precede_any_device_call(entries):
    """Host arrays stand in for device buffers: no refused call reaches a device."""
    raw = (ctypes.c_char * (4096 + 16))()
    p = (ctypes.addressof(raw) + 15) & ~15
    layout = dict(numel=16, nt=2, offsets=a([0, 8]), ks=a([3, 3]), k_off=a([0, 3]))
    nt = 70  # a bad tensor in the second batch of 64 is found before the first batch is launched
    ks = [1] * 69 + [9]
    bad_layouts = [dict(**{name: None}) for name in ("offsets", "ks", "k_off")]
    bad_layouts += [dict(nt=0), dict(numel=0), dict(ks=a([3, 9])), dict(ks=a([0, 3])),
                    dict(numel=12, offsets=a([0, 12])), dict(offsets=a([8, 0])),
                    dict(numel=2 * nt, nt=nt, offsets=a(range(0, 2 * nt, 2)), ks=a(ks), k_off=a(range(nt)))]
    wire = dict(packed_len=6, wire=p + 1024, stride=32)
    good = {NAMES[0]: dict(layout),
            NAMES[1]: dict(layout, idx=p, wire=p + 1024, stream=None),
            NAMES[2]: dict(layout, **wire, nranks=1, idx_out=p, stream=None),
            NAMES[3]: dict(out=p, **layout, **wire, vals=p + 2048, val_dtype=N.BF16, nranks=1, world_size=1,
                           gE=p + 3072, decay=1.0, stream=None)}
    bad = {NAMES[0]: [], NAMES[1]: [dict(idx=None), dict(wire=None), dict(wire=p + 1026)],
           NAMES[2]: [dict(wire=None), dict(idx_out=None), dict(nranks=0), dict(packed_len=7), dict(stride=31)],
           NAMES[3]: [dict(out=None), dict(wire=None), dict(vals=None), dict(nranks=0), dict(world_size=0),
                      dict(val_dtype=2), dict(vals=p + 2049), dict(gE=p + 3074), dict(stride=28),
                      dict(numel=24, offsets=a([8, 16]))]}  # a layout that does not start at 0
    for name, fn in entries.items():
        refused = -N.EINVAL if name == NAMES[0] else N.EINVAL
        for kw in bad_layouts + bad[name]:
            assert fn(*{**good[name], **kw}.values()) == refused, (name, kw)
    assert entries[NAMES[0]](*good[NAMES[0]].values()) == 32
    assert not any(raw.raw)


@pytest.mark.parametrize("cls", [SH.SparseState, SH4.SparseState])
def test_option_parsing_and_refusals(cls, monkeypatch):
    monkeypatch.delenv("ARCTOPK_SPARSE_INDEX_WIRE", raising=False)
    st = cls(None, sparse_type="tensor")
    assert st.index_wire is None and st.idx16_calls == 0 and not st._idx16()
    assert st.state_dict()["index_wire"] is None
    st.index_wire = "idx16"
    assert st._idx16() and st.state_dict()["index_wire"] == "idx16"
    st.sparse_type = "row"
    assert st._idx16()
    st.sparse_type = "column"
    with pytest.raises(ValueError, match="column"):
        st._idx16()
    st.random = True  # RandK sends no index: ignored, the column layout included
    assert not st._idx16()
    st.random = False
    for bad_value in ("idx8", 16, torch.int16):
        st.index_wire = bad_value
        with pytest.raises(ValueError, match="index_wire"):
            st._idx16()
    monkeypatch.setenv("ARCTOPK_SPARSE_INDEX_WIRE", "idx16")
    st = cls(None, use_error_feedback="ef21")
    assert st.index_wire == "idx16"
    st.large_batch_init = True
    hook = SH4.sparse_hook_sync if cls is SH4.SparseState else SH.sparse_hook_sync
    with pytest.raises(ValueError, match="large_batch_init"):
        hook(st, SyntheticBucket(torch.zeros(8), [[8]], index=0, is_last=True))
    monkeypatch.setenv("ARCTOPK_SPARSE_INDEX_WIRE", "IDX16")
    with pytest.raises(ValueError, match="ARCTOPK_SPARSE_INDEX_WIRE"):
        cls(None)


@pytest.mark.parametrize("ws", [1, 2, 4])
@pytest.mark.parametrize("value_bits", [16, 32])
def test_bit_formula(ws, value_bits, monkeypatch):
    """(ws - 1) ws (sum_k (value_bits + 16) + 32 blocks): the format's information bits."""
    monkeypatch.setattr(SH, "_all_gather_flat", lambda out, inp, group, world_size: None)
    st = SH.SparseState(None)
    numels, ks = [5, 65537, 131073], [1, 16384, 32768]
    wire = torch.zeros(F.wire_bytes(numels, ks), dtype=torch.uint8)
    values, indices = torch.zeros(sum(ks)), torch.zeros(sum(ks), dtype=torch.int32)
    _, idx, nranks, acc = SH._exchange(st, None, ws, values, indices, value_bits, True, hashed=False, by_column=False,
                                       idx16=(wire, F.blocks(numels)))
    assert F.blocks(numels) == 6 and (nranks, acc) == (ws, 1)
    assert idx.dtype == torch.uint8 and idx.numel() == ws * wire.numel()
    assert st.comm_bits_this_round == (ws - 1) * ws * (sum(ks) * (value_bits + 16) + 32 * 6)
