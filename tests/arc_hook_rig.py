"""A CPU rig that records which native calls and collectives the ARC-TopK hook makes.

The buckets live in CPU tensors, the process group is a stand-in of size 1 or 2, libarctopk is an
object that records every call (all arguments, by the parameter names of include/arctopk.h) and
returns 0 or a status set per call, plans are stubs that hold what the hook touches of a
BucketPlan, and the streams, communicators and events are recognisable stand-ins.  Nothing is
computed: what is pinned is the order of the calls, every scalar, which buffer, plan, stream or
marker array each pointer is (by role, never by value) and what a call leaves in the state.

tests/test_arc_hook_calls_host.py holds the matrix of cases, checks it against the rules of the hook's
comments and, run as a script, prints the whole matrix's trace as JSON lines for comparing two trees."""
import contextlib
import ctypes
import os
import types

import pytest
import torch
import torch.distributed as dist

from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import SyntheticBucket, bucket_numel
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape as H
from allreducetopk_amd.comm_hooks import group_topk_hook_no_reshape_c4 as H4

SHAPES = [[8, 64], [16]]  # the smallest layout with a sketch segment and a raw one
BUCKETS = [SHAPES, [[16, 64], [16]], [[16, 64], [32]]]  # a backward: bucket 0 is the smallest
RATIO, RANK, SEED = 0.2, 4, 7
STREAMS = {0x5712: "caller", 0x5713: "caller2", 0xA0: "ar", 0xB0: "sel0", 0xB1: "sel1", 0xC0: "copy", 0xD0: "side"}
COMMS = {0x51: "sk", 0x52: "pk"}
GROUPS = {2: ((0, 0), (256, 64)), 3: ((0, 0), (128, 32), (384, 96))}  # (offset, v_off) of the stub groups
_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.int32: "i32"}
ENV = "ARCTOPK_"

# parameter names of the entry points the hook calls (include/arctopk.h)
ARGS = {
    "arctopk_exchange_step": "plan bucket err gerr ef err_in draw seed next next_seed sketch_comm packed_comm stream "
                             "ar_stream defer ride ride_marks finish finish_marks nfinish V marks sel_stream trail",
    "arctopk_exchange_trail": "plan bucket err gerr ef err_in draw seed V stream",
    "arctopk_exchange_finish": "plan stream marks",
    "arctopk_plan_bind_wire16": "plan packed_bf16",
    "arctopk_encode_mixed": "plan grad_bf16 err_f32 err_in V_bf16 sketch_bf16 stream",
    "arctopk_pack_mixed": "plan grad_bf16 err_f32 err_in rowlist slotmap packed_bf16 stream",
    "arctopk_encode_mixed21": "plan grad_bf16 err_f32 V_bf16 sketch_bf16 stream",
    "arctopk_pack_mixed21": "plan grad_bf16 err_f32 rowlist slotmap packed_bf16 stream",
    "arctopk_decode_mixed21": "plan packed_bf16 slotmap world_size gerr_f32 out_bf16 stream",
    "arctopk_pack_wire16": "plan grad err ef err_in rowlist slotmap packed_bf16 stream",
    "arctopk_decode_wire16": "plan packed_bf16 slotmap world_size ef gerr out stream",
    "arctopk_comm_allreduce": "comm buf count dtype stream",
    "arctopk_draw_projections": "plan seed V stream",
}


class Event:
    """Stands in for N.DeviceEvent (a timing marker)."""
    count = 0

    def __init__(self, timing=False):
        Event.count += 1
        self.handle = 0xE000 + Event.count
        self.rec = None

    def record(self, stream):
        self.rec.trace.append({"event": "record", "stream": self.rec.role(stream)})


class Comm:
    """Stands in for an exchange.Comm: records what is registered and checked."""
    kind = "rccl"

    def __init__(self, rec, handle):
        self.rec, self.handle, self.registered = rec, handle, []

    def register(self, t):
        self.registered.append(t)
        self.rec.trace.append({"comm": COMMS[self.handle], "op": "register", "buf": self.rec.role(t.data_ptr())})

    def check(self, status, what):
        self.rec.trace.append({"comm": COMMS[self.handle], "op": "check", "status": int(status)})
        N.check(status, what)

    def raise_if_failed(self):
        pass


class Group(H.GroupPlan):
    """What the hook touches of a GroupPlan (an instance, so that _bucket_plan_of finds its parent)."""

    def __init__(self, parent, i, offset, v_off):
        self.parent = lambda: parent
        self.handle = parent.handle + 1 + i
        self.offset, self.v_off = offset, v_off
        self.sketch, self.packed = parent.sketch[8 * i:], parent.packed[8 * i:]
        self.comm_registered = self.v_drawn = self.v_stream = None

    def __del__(self):  # (no native plan behind it)
        pass


class Plan:
    """What the hook touches of a BucketPlan; geometry by the plan's own rules, buffers on the CPU."""

    def __init__(self, rec, b, shapes, ratio, dtype, flags=0):
        self.rec, self.b, self.r, self.ratio, self.dtype, self.flags = rec, b, RANK, ratio, dtype, flags
        self.device = torch.device("cpu")
        self.handle = 0x100000 * (len(rec.plans) + 1)
        self.segments = []
        for s in shapes:
            kind, n, m = H._geometry(s)
            if kind == N.SEG_RAW and flags & N.PLAN_DENSE_1D:
                kind = N.SEG_DENSE
            k_rows = n if kind == N.SEG_DENSE else max(1, int(n * ratio))
            self.segments.append(types.SimpleNamespace(kind=kind, n=n, m=m, k_rows=k_rows))
        sk = [s for s in self.segments if s.kind == N.SEG_SKETCH]
        self.ms = tuple(s.m for s in sk)
        values = sum(s.k_rows * s.m for s in self.segments)
        self.info = types.SimpleNamespace(
            numel=bucket_numel(shapes), v_len=sum(self.ms) * RANK, values_len=values, packed_len=-(-values // 16) * 16,
            sketch_len=sum(s.n * RANK for s in sk) + sum(s.n for s in self.segments if s.kind == N.SEG_RAW))
        self.slotmap = torch.zeros(sum(s.n for s in self.segments), dtype=torch.int32)
        self.rowlist = torch.zeros(sum(s.k_rows for s in self.segments), dtype=torch.int32)
        self.sketch = torch.zeros(self.info.sketch_len, dtype=dtype)
        self.packed = torch.zeros(self.info.packed_len, dtype=dtype)
        self.V_ring = [torch.zeros(self.info.v_len, dtype=dtype)]
        self.sketch_view, self.packed_view = self.sketch, self.packed
        self.bits_sum = H.BucketPlan.bits_of(self.segments, RANK, dtype)
        self.philox_advance = 0
        self.comm_registered = self.packed16 = self.packed16_registered = None
        self.wire16_bound = False
        self.v_drawn = self.v_stream = self.prestaged = None
        self._groups = None

    def groups(self, target_bytes):
        if self._groups is None:
            self._groups = [Group(self, i, off, voff) for i, (off, voff) in enumerate(GROUPS[self.rec.ngroups or (3 if self.b == 1 else 2)])]
        return self._groups

    def _note(self, name, **kw):
        role = self.rec.role
        self.rec.trace.append({"plan_call": name, "plan": role(self.handle),
                               **{k: role(v.data_ptr()) if isinstance(v, torch.Tensor) else v for k, v in kw.items()}})

    def encode(self, grad, err, ef, err_in, V, stream):
        self._note("encode", grad=grad, err=self.rec.role(N.ptr(err)), ef=ef, err_in=int(err_in), V=V,
                   stream=self.rec.role(stream))

    def select(self, world_size, stream, next_plan=None, next_seed=0):
        self._note("select", world_size=world_size, stream=self.rec.role(stream),
                   next=self.rec.role(next_plan.handle if next_plan is not None else None), next_seed=int(next_seed))

    def pack(self, grad, err, ef, stream):
        self._note("pack", grad=grad, err=self.rec.role(N.ptr(err)), ef=ef, stream=self.rec.role(stream))

    def decode(self, world_size, ef, gerr, out, stream):
        self._note("decode", world_size=world_size, ef=ef, gerr=self.rec.role(N.ptr(gerr)), out=out,
                   stream=self.rec.role(stream))

    def projection_consumed(self, i, stream):
        self._note("projection_consumed", slot=int(i), stream=self.rec.role(stream.cuda_stream))


class Recorder:
    """Stands in for libarctopk, and keeps the trace of one case's calls."""

    def __init__(self):
        self.trace = []
        self.bucket = None      # the bucket of the hook call in progress
        self.state = None
        self.stream = 0x5712    # what _current_raw_stream answers
        self.status = {}        # entry point -> a status for every call, or a list consumed call by call
        self.plans = {}         # (id(state), bucket, dtype, ratio, flags) -> Plan
        self.marks = []         # every marker array a hook call made
        self.host_v = 0         # the ring slot a patched _host_projections hands out
        self.ngroups = None     # groups per bucket (default: three for bucket 1, two for the others)

    def plan_role(self, p):
        for plan in self.plans.values():
            if plan.handle == p:
                return f"plan[{plan.b}]"
            if plan.handle < p <= plan.handle + 3:
                return f"plan[{plan.b}].group[{p - plan.handle - 1}]"
        return None

    def role(self, a):
        if isinstance(a, ctypes.Array):
            for i, m in enumerate(self.marks):
                if m is a:
                    return f"marks[{i}]"
            return [self.role(v) for v in a]
        p = int(getattr(a, "value", a) or 0)
        if p == 0:
            return "NULL"
        if p in STREAMS or p in COMMS:
            return STREAMS.get(p) or COMMS[p]
        if self.plan_role(p):
            return self.plan_role(p)
        for i, m in enumerate(self.marks):
            if ctypes.addressof(m) == p:
                return f"marks[{i}]"
        st, b = self.state, self.bucket.index()
        plan = st._plans[b][1] if b in st._plans else None
        named = [("bucket", self.bucket.buffer()), ("error_dict[b]", st.error_dict.get(b)),
                 ("global_error_dict[b]", st.global_error_dict.get(b))]
        if plan is not None:
            named += [("V", plan.V_ring[0]), ("packed16", plan.packed16), ("packed", plan.packed),
                      ("sketch", plan.sketch), ("rowlist", plan.rowlist), ("slotmap", plan.slotmap)]
        for name, t in named:
            if t is not None and t.data_ptr() <= p < t.data_ptr() + max(1, t.numel() * t.element_size()):
                off = p - t.data_ptr()
                return f"{name}+{off}" if off else name
        return "unknown"

    def __getattr__(self, name):
        if not name.startswith("arctopk_"):
            raise AttributeError(name)
        names = ARGS[name].split()
        types_ = N._SIGS[name][1]

        def fn(*args):
            assert len(args) == len(names) == len(types_), name
            rec = {}
            for key, ty, a in zip(names, types_, args):
                rec[key] = self.role(a) if ty is ctypes.c_void_p else float(a) if ty is ctypes.c_double else int(a)
            self.trace.append({"call": name, **rec})
            status = self.status.get(name, 0)
            if isinstance(status, list):
                status = status.pop(0) if status else 0
            return status

        return fn

    # torch's process group: the warm-up's and EF21's first call's all-reduces, host_staged's at world size > 1
    def all_reduce(self, tensor, group=None, async_op=False):
        self.trace.append({"coll": "all_reduce", "dtype": _DT[tensor.dtype], "numel": tensor.numel(),
                           "buf": self.role(tensor.data_ptr()), "async_op": bool(async_op)})
        if async_op:
            fut = torch.futures.Future()
            fut.set_result([tensor])
            return types.SimpleNamespace(get_future=lambda: fut)


@contextlib.contextmanager
def patched(rec: Recorder):
    """libarctopk, the stream query, the global reseed, the events and torch's collectives replaced by
    ``rec``'s; the host projections (pinned memory, a copy stream) and the host-staged copy record only."""
    def current_raw_stream(dix):
        return rec.stream

    def call_marks(state, names, real=H._call_marks):
        arr = real(state, names)
        if arr is not None:
            rec.marks.append(arr)
        return arr

    def event(timing=False):
        e = Event(timing)
        e.rec = rec
        return e

    def host_projections(state, plan, bucket, seed, dtype, dev, stream):
        rec.trace.append({"host_projections": rec.role(plan.handle), "seed": int(seed),
                          "stream": rec.role(stream.cuda_stream)})
        return rec.host_v, plan.V_ring[0]

    def stage_through_host(state, pv, stream, dev, chunks=8):
        rec.trace.append({"stage_through_host": rec.role(pv.data_ptr()), "stream": rec.role(stream.cuda_stream)})

    new = [(N, "lib", lambda: rec), (H, "_LIB", [rec]), (H, "_reseed_global", lambda *a, **k: None),
           (H, "_current_raw_stream", current_raw_stream), (H, "_call_marks", call_marks), (N, "DeviceEvent", event),
           (H, "_host_projections", host_projections), (H, "_stage_through_host", stage_through_host),
           (dist, "all_reduce", rec.all_reduce),
           (torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=rec.stream)),
           (torch.cuda, "synchronize", lambda device=None: rec.trace.append({"synchronize": str(device)}))]
    saved = [(obj, name, getattr(obj, name)) for obj, name, _ in new]
    rec.real_lib = N.lib  # (for a test that builds its plans' geometry with the library itself)
    for obj, name, val in new:
        setattr(obj, name, val)
    try:
        yield
    finally:
        for obj, name, val in saved:
            setattr(obj, name, val)


def make_state(rec, cls=H.GroupTopKState, ef="ef14", ws=1, r=RANK, **kw):
    """A state whose plans are stubs and whose communicators and streams are the rig's stand-ins (the
    tables the state's own _exchange_comms, _side_stream and _select_stream look them up in)."""
    group = types.SimpleNamespace(size=lambda: ws)
    st = cls(group, r=r, compress_ratio=RATIO, start_compress_iter=0, use_error_feedback=ef, seed=SEED, **kw)
    ns = types.SimpleNamespace

    def plan_for(bucket, buf=None):
        buf = bucket.buffer() if buf is None else buf
        key = (id(st), bucket.index(), buf.dtype, st._plan_ratio(), st._plan_flags())
        if key not in rec.plans:
            rec.plans[key] = Plan(rec, bucket.index(), [tuple(g.shape) for g in bucket.gradients()], key[3], buf.dtype,
                                  key[4])
        st._plans[bucket.index()] = (key, rec.plans[key], None)  # (_next_plan reads it)
        return rec.plans[key]

    st._plan_for = plan_for
    st._comms = (group, torch.device("cpu"), Comm(rec, 0x51), Comm(rec, 0x52))
    st._ar_streams[0], st._copy_streams[0], st._side_streams[0] = ns(cuda_stream=0xA0), ns(cuda_stream=0xC0), ns(cuda_stream=0xD0)
    st._sel_streams[0] = [ns(cuda_stream=0xB0), ns(cuda_stream=0xB1)]
    rec.state = st
    return st


def hook_call(rec, st, b=0, dtype=torch.float32, shapes=SHAPES, is_last=True, hook=H.group_topk_hook):
    """One hook call on a fresh bucket tensor: (its Future, the records of what it called)."""
    rec.trace = []
    rec.bucket = SyntheticBucket(torch.ones(bucket_numel(shapes), dtype=dtype), shapes, index=b, is_last=is_last)
    return hook(st, rec.bucket), rec.trace


def brief(trace, fields):
    """The native calls and plan calls of ``trace`` as tuples (name without "arctopk_", then the record's
    values of ``fields[name]``): what the path tests compare."""
    out = []
    for t in trace:
        name = (t.get("call") or t.get("plan_call") or "")[len("arctopk_") if "call" in t else 0:]
        if name and name not in ("projection_consumed", "draw_projections"):  # (the projections' plumbing)
            out.append((name,) + tuple(t[k] for k in fields.get(name, ())))
    return out


@pytest.fixture()
def rig(monkeypatch):
    """The rig for one test: ``make`` a state (select streams off, nothing deferred, no trailing step unless
    the test sets them) and ``call`` the hook: (its Future, the records).  ``brief(fields, ...)``: the same
    with other defaults, whose ``call`` checks whether the Future is done, keeps it in ``fut`` and returns
    the calls as brief(trace, fields)."""
    for v in [v for v in os.environ if v.startswith(ENV)]:
        monkeypatch.delenv(v)
    rec = Recorder()
    ns = types.SimpleNamespace(rec=rec, plan=lambda st, b=0: st._plans[b][1])

    def make(cls=H.GroupTopKState, ef="ef14", ws=1, **kw):
        st = make_state(rec, cls, ef, ws, **kw)
        st.select_streams, st.defer_decode, st.trail_bytes = "off", False, 0
        return st

    def call(st, dtype=torch.float32, b=0, hook=H.group_topk_hook, is_last=True, shapes=SHAPES):
        rec.state = st
        return hook_call(rec, st, b, dtype, shapes, is_last, hook)

    def brief_rig(fields, dtype=torch.float32, ef="ef14"):
        def brief_call(st, dtype=dtype, done=True, **kw):
            out.fut, trace = call(st, dtype=dtype, **kw)
            assert out.fut.done() == done
            return brief(trace, fields)

        out = types.SimpleNamespace(rec=rec, plan=ns.plan, call=brief_call,
                                    make=lambda cls=H.GroupTopKState, ef=ef, **kw: make(cls, ef, **kw))
        return out

    ns.make, ns.call, ns.brief = make, call, brief_rig
    with patched(rec):
        yield ns


# ---- the matrix ------------------------------------------------------------------------------------
VARIANTS = {"fp32": {}, "bf16": {}, "bf16+error_dtype": {"error_dtype": torch.float32},
            "bf16+ef21_error_dtype": {"ef21_error_dtype": torch.float32},
            "fp32+wire_dtype": {"wire_dtype": torch.bfloat16},
            "fp32+wire_dtype+step": {"wire_dtype": torch.bfloat16, "wire_exchange": "step"}}
WORLDS = {"ws1": (1, False), "ws2": (2, False), "ws1force": (1, True)}
BACKWARD = [("hook", 0), ("hook", 1), ("hook", 2, True)]


def snapshot(rec, st, futs) -> dict:
    """What a step leaves in the state."""
    zr = {int(b): bool(r[0] is st._plans[b][1] and r[1] is st.error_dict.get(b)) for b, r in st._zr.items()}
    return {"iter": int(st.iter), "comm_bits_this_round": int(st.comm_bits_this_round),
            "mixed_calls": int(st.mixed_calls), "wire16_calls": int(st.wire16_calls),
            "wire16_step_calls": int(st.wire16_step_calls), "trail_calls": int(st.trail_calls),
            "pend": [rec.role(e[0].handle) for e in st._x_pend],
            "trail": None if st._trail is None else rec.role(st._trail[0].handle),
            "sel_small": st._sel_small, "sel_small_last": st._sel_small_last, "sel_turn": st._sel_turn,
            "futures_done": [bool(f.done()) for f in futs],
            "error_dtype": {int(b): _DT[t.dtype] for b, t in st.error_dict.items()},
            "global_error_dtype": {int(b): _DT[t.dtype] for b, t in st.global_error_dict.items()},
            "zero_rows": zr, "wire16_bound": {int(b): bool(p[1].wire16_bound) for b, p in sorted(st._plans.items())}}


def run_case(ef="ef14", variant="fp32", world="ws1", c4=False, script=None, buckets=BUCKETS, ngroups=None, **opts):
    """The steps of one fresh state, each the records of what it called, ending in the state's snapshot
    (or the exception's name).  ``script``: ("hook", bucket[, is_last]), ("stream", handle),
    ("status", entry point, statuses), ("set", attribute, value), ("wait", index of a Future handed out);
    default: two backwards of three buckets (three with EF21, whose first is dense)."""
    saved_env = {v: os.environ.pop(v) for v in list(os.environ) if v.startswith(ENV)}
    rec = Recorder()
    rec.ngroups = ngroups
    Event.count = 0
    ws, force = WORLDS[world]
    dtype = torch.float32 if variant.startswith("fp32") else torch.bfloat16
    hook = H4.group_topk_hook if c4 else H.group_topk_hook
    script = script or BACKWARD * (3 if ef == "ef21" else 2)
    out, futs = [], []
    try:
        with patched(rec):
            st = make_state(rec, H4.GroupTopKState if c4 else H.GroupTopKState, ef, ws)
            st.force_exchange, st.defer_decode = force, True
            for k, v in {**VARIANTS[variant], **opts}.items():
                setattr(st, k, v)
            for step in script:
                rec.trace = []
                if step[0] == "stream":
                    rec.stream = step[1]
                    continue
                if step[0] == "status":
                    rec.status[step[1]] = list(step[2])
                    continue
                if step[0] == "set":
                    setattr(st, step[1], step[2])
                    continue
                try:
                    if step[0] == "wait":
                        futs[step[1]].wait()
                    else:
                        b, last = step[1], len(step) > 2 and step[2]
                        futs.append(hook_call(rec, st, b, dtype, buckets[b], last, hook)[0])
                except (RuntimeError, ValueError) as e:
                    rec.trace.append({"raised": type(e).__name__})
                out.append({"step": list(step), "trace": rec.trace, "state": snapshot(rec, st, futs)})
    finally:
        os.environ.update(saved_env)
    return out
