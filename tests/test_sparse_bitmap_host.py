"""``SparseState.index_wire = "bitmap"`` / ``"auto"`` on the CPU: the format's size, the four C entries'
refusals (which precede any device call), the option's parsing, the bit formula and "auto"'s choice.

(The kernels and the hooks on a GPU: tests/test_gpu_sparse_bitmap.py.)"""
import ctypes
import os

import pytest
import torch

import sparse_bitmap_format as F
import sparse_idx16_format as F16
import test_sparse_idx16_host as I
from allreducetopk_amd import _native as N
from allreducetopk_amd.build import LIB, build
from allreducetopk_amd.comm_hooks import sparse_hook as SH
from allreducetopk_amd.comm_hooks import sparse_hook_c4 as SH4

a = N.i64_array
NAMES = ("arctopk_sparse_bitmap_bytes", "arctopk_sparse_bitmap_pack", "arctopk_sparse_bitmap_unpack",
         "arctopk_sparse_decode_bitmap")
C = 4096


@pytest.fixture(scope="module")
def entries():
    if not os.path.exists(LIB):
        build()
    L = ctypes.CDLL(LIB)
    fns = {}
    for name in NAMES + ("arctopk_sparse_idx16_bytes",):
        fns[name] = getattr(L, name)
        fns[name].restype, fns[name].argtypes = N._SIGS[name]
    return fns


def _lay(numels, ks):
    return (sum(numels), len(numels), a([sum(numels[:i]) for i in range(len(numels))]), a(ks),
            a([sum(ks[:i]) for i in range(len(ks))]))


@pytest.mark.parametrize("numels,ks", [([31, 32, 33, C - 1, C, C + 1, 2 * C + 1], [7, 8, 8, 1023, 1024, 1024, 2048]),
                                       ([C + 1], [C + 1]), ([3 * C + 5], [3]), ([33] * 70, [8] * 70), ([1], [1]),
                                       ([2 ** 31 - 1], [3])])
def test_bytes(entries, numels, ks):
    got = entries[NAMES[0]](*_lay(numels, ks))
    assert got == F.wire_bytes(numels, ks) and got % 16 == 0 and 8 * got >= F.info_bits(numels)


def test_refusals_precede_any_device_call(entries, monkeypatch):
    """The four entries take their idx16 counterparts' arguments, so that test's list of bad arguments runs
    on them as it stands: every refusal is EINVAL (-EINVAL from _bytes) and no host stand-in buffer is touched."""
    monkeypatch.setattr(I, "NAMES", NAMES)
    I.test_refusals_precede_any_device_call({name: entries[name] for name in NAMES})


@pytest.mark.parametrize("cls", [SH.SparseState, SH4.SparseState])
def test_option_parsing(cls, monkeypatch):
    monkeypatch.delenv("ARCTOPK_SPARSE_INDEX_WIRE", raising=False)
    st = cls(None, sparse_type="tensor")
    assert st.bitmap_calls == 0
    for value in ("bitmap", "auto"):
        st.index_wire, st.sparse_type, st.random = value, "row", False
        assert st._idx16() == value and st.state_dict()["index_wire"] == value
        st.sparse_type = "column"
        with pytest.raises(ValueError, match="column"):
            st._idx16()
        st.random = True  # RandK sends no index
        assert st._idx16() is None
        monkeypatch.setenv("ARCTOPK_SPARSE_INDEX_WIRE", value)
        assert cls(None).index_wire == value
    for bad_value in ("Bitmap", "bits", ("bitmap",)):
        st.index_wire, st.random = bad_value, False
        with pytest.raises(ValueError, match="index_wire"):
            st._idx16()
    monkeypatch.setenv("ARCTOPK_SPARSE_INDEX_WIRE", "bitmap,auto")
    with pytest.raises(ValueError, match="ARCTOPK_SPARSE_INDEX_WIRE"):
        cls(None)


class _Lib:
    """The two *_bytes entries from the real library, every other entry a recorded no-op."""

    def __init__(self, entries):
        self.entries, self.calls = entries, []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return self.entries[name](*args) if name.endswith("_bytes") else 0
        return fn


@pytest.mark.parametrize("ws", [1, 2, 4])
@pytest.mark.parametrize("value_bits", [16, 32])
def test_bit_formula(entries, ws, value_bits, monkeypatch):
    """(ws - 1) ws (sum_k value_bits + sum_i (n_i + 32 nc_i)), through _index_pack and _exchange."""
    monkeypatch.setattr(SH, "_all_gather_flat", lambda out, inp, group, world_size: None)
    st = SH.SparseState(None)
    numels, ks = [5, C + 1, 3 * C], [1, 1024, 3000]
    values, indices = torch.zeros(sum(ks)), torch.zeros(sum(ks), dtype=torch.int32)
    fmt, packed = SH._index_pack(_Lib(entries), _lay(numels, ks), indices, numels, "bitmap", None)
    assert fmt == "bitmap" and packed[0].numel() == F.wire_bytes(numels, ks)
    _, idx, nranks, acc = SH._exchange(st, None, ws, values, indices, value_bits, True, hashed=False, by_column=False,
                                       idx16=packed)
    assert (nranks, acc) == (ws, 1) and idx.dtype == torch.uint8 and idx.numel() == ws * packed[0].numel()
    assert F.info_bits(numels) == 5 + C + 1 + 3 * C + 32 * 6
    assert st.comm_bits_this_round == (ws - 1) * ws * (sum(ks) * value_bits + F.info_bits(numels))


@pytest.mark.parametrize("numels,ks,want", [
    ([65536], [4096], "idx16"),      # ratio 1/16: 8192 + 16 B of idx16 against 8192 + 64 B of bitmap
    ([65536], [4128], "bitmap"),     # 64 B of indices more: 8272 against 8256
    ([65536], [4120], "idx16"),      # 8256 against 8256: a tie goes to idx16
    ([2048 * 2048] * 2, [83886] * 2, "idx16"), ([2048 * 2048] * 2, [838860] * 2, "bitmap"),  # ratios 0.02 and 0.2
])
def test_auto_takes_the_smaller_payload(entries, numels, ks, want):
    lib = _Lib(entries)
    lay = _lay(numels, ks)
    fmt, packed = SH._index_pack(lib, lay, torch.zeros(sum(ks), dtype=torch.int32), numels, "auto", None)
    sizes = {"idx16": F16.wire_bytes(numels, ks), "bitmap": F.wire_bytes(numels, ks)}
    assert fmt == want == min(sizes, key=sizes.get) and packed[0].numel() == sizes[want]
    assert lib.calls == ["arctopk_sparse_idx16_bytes", "arctopk_sparse_bitmap_bytes", f"arctopk_sparse_{want}_pack"]
