"""Which native calls and collectives the ARC-TopK hook makes, on the CPU (arc_hook_rig): the rules of
the hook's comments and GroupTopKState's docstrings restated as a small model of the pending FIFO and
checked call by call -- ride depth, who finishes whom, which Futures are done when, when everything
pending is flushed, trailing steps, exchange groups, select streams, the ``err_in`` code, the seed and
the pre-drawn projections, which buffer each pointer is and the ``comm_bits_this_round`` arithmetic.
The expectations are written from those rules, not from a recorded run.

``python tests/test_arc_hook_calls_host.py`` prints the matrix's whole trace as sorted JSON lines.

(What the kernels compute: tests/test_gpu_arctopk.py and the other GPU tests; that the real library is
called as the rig's stub is: tests/test_gpu_configs.py::test_real_calls_match_the_rig.)"""
import itertools
import json
import os
import sys

import pytest
import torch

if __name__ == "__main__":  # (the dump, run as a script from anywhere: the package is the repository's)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import arc_hook_rig as R
from allreducetopk_amd import _native as N
from allreducetopk_amd.bucket import bucket_numel


def trail_bytes(variant="fp32"):
    """A trail_bytes that only bucket 0 fits under."""
    return bucket_numel(R.BUCKETS[0]) * (4 if variant.startswith("fp32") else 2)


def matrix():
    """(case id, arguments of run_case) of everything the test and the dump cover."""
    # paths: the defaults of a deferring caller (trailing steps, "auto" groups and select streams)
    for ef, variant, world in itertools.product(("noef", "ef14", "ef21"), R.VARIANTS, R.WORLDS):
        yield f"path-{ef}-{variant}-{world}", dict(ef=ef, variant=variant, world=world)
    plain = dict(trail_bytes=0, select_streams="off", exchange_groups="off")
    yield "warmup-with-pending-ws1", dict(script=[("hook", 0), ("set", "start_compress_iter", 5), ("hook", 1), ("hook", 2, True)], **plain)
    yield "warmup-ws2", dict(world="ws2", script=[("set", "start_compress_iter", 1)] + R.BACKWARD * 2)
    # deferral
    for dd, world in itertools.product((True, False, None), ("ws1", "ws2")):
        yield f"defer-{dd}-{world}", dict(world=world, defer_decode=dd, **plain)
        yield f"defer-{dd}-{world}-marks", dict(world=world, defer_decode=dd, phase_events=[], **plain)
    yield "defer-sync-exchange-ws2", dict(world="ws2", async_exchange=False, **plain)
    for world in ("ws1", "ws2"):
        yield f"wait-first-{world}", dict(world=world, script=[("hook", 0), ("hook", 1), ("wait", 0), ("hook", 2, True)], **plain)
        # flush conditions
        yield f"same-bucket-again-{world}", dict(world=world, script=[("hook", 0), ("hook", 1), ("hook", 0), ("hook", 2, True)], **plain)
        yield f"stream-change-{world}", dict(world=world, script=[("hook", 0), ("stream", 0x5713), ("hook", 1), ("hook", 2, True)], **plain)
        yield f"skipped-bucket-{world}", dict(world=world, script=R.BACKWARD + [("hook", 0), ("hook", 2, True)] + R.BACKWARD, **plain)
    # trailing steps
    tb = dict(trail_bytes=trail_bytes(), select_streams="off")
    for name, status in (("ok", 0), ("einval", N.EINVAL), ("fails", 700)):
        yield f"trail-{name}", dict(script=[("status", "arctopk_exchange_trail", [status])] + R.BACKWARD * 2, **tb)
    yield "trail-noef", dict(ef="noef", **tb)
    yield "trail-host-projections", dict(projections="host", **tb)
    yield "trail-stream-change", dict(script=[("hook", 0), ("stream", 0x5713), ("hook", 1), ("hook", 2, True)], **tb)
    yield "trail-same-plan", dict(script=[("hook", 0), ("hook", 0), ("hook", 2, True)], **tb)
    yield "trail-then-wire16-step", dict(script=[("hook", 0), ("set", "wire_dtype", torch.bfloat16),
                                                 ("set", "wire_exchange", "step"), ("hook", 1), ("hook", 2, True)], **tb)
    yield "trail-then-last", dict(script=[("hook", 0), ("hook", 2, True)], **tb)
    yield "trail-wait", dict(script=[("hook", 0), ("wait", 0), ("hook", 1), ("hook", 2, True)], **tb)
    yield "no-trail-ef21", dict(ef="ef21", **tb)
    yield "no-trail-marks", dict(phase_events=[], **tb)
    yield "no-trail-ws2", dict(world="ws2", **tb)
    yield "no-trail-force", dict(world="ws1force", **tb)
    yield "no-trail-select-on", dict(trail_bytes=trail_bytes(), select_streams="on")
    # groups
    for groups, proj, world in itertools.product(("off", "auto", "all"), ("device", "host"), ("ws2", "ws1force")):
        yield f"groups-{groups}-{proj}-{world}", dict(world=world, exchange_groups=groups, projections=proj,
                                                      trail_bytes=0, select_streams="off")
    yield "groups-all-ef21-ws2", dict(ef="ef21", world="ws2", exchange_groups="all", trail_bytes=0, select_streams="off")
    yield "groups-all-ws1", dict(exchange_groups="all", trail_bytes=0, select_streams="off")  # (no collectives: whole buckets)
    yield "groups-all-marks-ws2", dict(world="ws2", exchange_groups="all", phase_events=[], trail_bytes=0, select_streams="off")
    # select streams
    for world in R.WORLDS:
        yield f"select-on-{world}", dict(world=world, select_streams="on", trail_bytes=0, exchange_groups="off")
        yield f"select-auto-{world}", dict(world=world, select_streams="auto", select_stream_min_buckets=3, trail_bytes=0,
                                           exchange_groups="off", script=R.BACKWARD * 3)
    yield "select-on-no-defer", dict(select_streams="on", defer_decode=False, trail_bytes=0)
    yield "select-on-groups-all-ws2", dict(world="ws2", select_streams="on", exchange_groups="all", trail_bytes=0)
    # failures of the step
    for world in ("ws1", "ws2"):
        yield f"step-fails-{world}", dict(world=world, script=[("hook", 0), ("status", "arctopk_exchange_step", [N.EINVAL]),
                                                               ("hook", 1), ("hook", 2, True)] + R.BACKWARD, **plain)
    # the host-staged measurement mode, with phase marks
    for proj, world in itertools.product(("device", "host"), ("ws1", "ws2")):
        yield f"host-staged-{proj}-{world}", dict(world=world, host_staged=True, phase_events=[], projections=proj)
    yield "host-staged-after-pending", dict(script=[("hook", 0), ("set", "host_staged", True), ("hook", 1), ("hook", 2, True)], **plain)
    # invalid options
    yield "raises-ef-name", dict(ef="ef15")
    yield "raises-wire-host-staged", dict(variant="fp32+wire_dtype", host_staged=True)
    yield "raises-wire-exchange", dict(variant="fp32+wire_dtype", wire_exchange="pipelined")
    # the c4 state and hook
    yield "c4-ef14-fp32-ws1", dict(c4=True)
    yield "c4-ef14-bf16+error_dtype-ws2", dict(c4=True, variant="bf16+error_dtype", world="ws2")
    yield "c4-ef14-fp32+wire_dtype+step-ws1force", dict(c4=True, variant="fp32+wire_dtype+step", world="ws1force")


MATRIX = list(matrix())
DEFAULTS = dict(defer_decode=True, async_exchange=True, trail_bytes=2 << 20, select_streams="auto",
                select_stream_min_buckets=4, exchange_groups="auto", projections="device", phase_events=None,
                host_staged=False, start_compress_iter=0, error_dtype=None, ef21_error_dtype=None, wire_dtype=None,
                wire_exchange="inline", err_zero_rows=True, select_stream_bytes=64 << 20)
PHASED = {  # path -> (encode, pack, decode, sketch wire, packed wire, packed buffer)
    "mixed": ("arctopk_encode_mixed", "arctopk_pack_mixed", "decode", N.BF16, N.BF16, "packed"),
    "mixed21": ("arctopk_encode_mixed21", "arctopk_pack_mixed21", "arctopk_decode_mixed21", N.BF16, N.BF16, "packed"),
    "wire16": ("encode", "arctopk_pack_wire16", "arctopk_decode_wire16", N.F32, N.BF16, "packed16")}


class Entry:
    """A pending step of the model: (plan role, bucket, stream role, marks role, index of its Future)."""

    def __init__(self, plan, b, stream, marks, fut):
        self.plan, self.b, self.stream, self.marks, self.fut = plan, b, stream, marks, fut


def plan_bits(shapes, bits, c4=False, wire16=False, ratio=R.RATIO):
    """bits_sum of one call: per tensor the sketch (n r values; a 1-D tensor's n; none for c4's dense 1-D)
    and k rows of m values; the bf16 wire counts the sketch in fp32 and the values in bf16."""
    sketch = values = 0
    for s in shapes:
        _, n, m = R.H._geometry(s)
        dense = c4 and len(s) == 1
        sketch += 0 if dense else n * R.RANK if len(s) > 1 else n
        values += (n if dense else max(1, int(n * ratio))) * m
    return sketch * 32 + values * 16 if wire16 else (sketch + values) * bits


class Model:
    """The hook's scheduling rules, applied to one case's steps."""

    def __init__(self, cid, ef="ef14", variant="fp32", world="ws1", c4=False, script=None, **opts):
        self.cid, self.ef, self.c4 = cid, ef, c4
        self.ws, force = R.WORLDS[world]
        self.o = {**DEFAULTS, **R.VARIANTS[variant], "force_exchange": force, **opts}
        self.f32 = variant.startswith("fp32")
        self.esz = 4 if self.f32 else 2
        self.stream = "caller"
        self.pend, self.trail, self.futs = [], None, []  # futs: per call "done", its pending Entry, "stuck" or "lost" (none handed out)
        self.seeds = torch.Generator().manual_seed(R.SEED)
        self.succ, self.last_b, self.planned = {}, None, set()
        self.v_drawn, self.v_stream = {}, {}
        self.residual, self.zr = set(), set()
        self.bits = self.iter = self.nmarks = 0
        self.sel_small = self.sel_small_last = self.sel_turn = 0
        self.count = dict(mixed_calls=0, wire16_calls=0, wire16_step_calls=0, trail_calls=0)
        self.bound = {}

    # ---- which path a call takes -----------------------------------------------------------------
    def path(self, b):
        o, bf16 = self.o, not self.f32
        if self.iter < o["start_compress_iter"]:
            return "warmup"
        if self.ef not in N.EF_CODE:
            return "ValueError"
        if bf16 and self.ef == "ef21" and o["error_dtype"] is not None and o["ef21_error_dtype"] is None:
            return "ValueError"  # error_dtype is EF14's
        wire16 = self.f32 and o["wire_dtype"] is not None
        if wire16 and o["host_staged"] or o["wire_exchange"] not in ("inline", "step"):
            return "ValueError"
        if self.ef == "ef21" and b not in self.residual:
            return "ef21-first"
        if bf16 and self.ef == "ef21" and o["ef21_error_dtype"] is not None:
            return "mixed21"
        if bf16 and self.ef == "ef14" and o["error_dtype"] is not None:
            return "mixed"
        if wire16 and o["wire_exchange"] == "inline":
            return "wire16"
        return "host_staged" if o["host_staged"] else "w16step" if wire16 else "step"

    # ---- the pending FIFO --------------------------------------------------------------------------
    def finish(self, t, where):
        """arctopk_exchange_finish: the oldest pending step, on the stream of its call, with its markers."""
        assert self.pend, f"{where}: a finish with nothing pending"
        e = self.pend.pop(0)
        assert (t["plan"], t["stream"], t["marks"]) == (e.plan, e.stream, e.marks), f"{where}: {t}"
        if e is self.trail:
            self.trail = None
        if e.fut is not None:
            self.futs[e.fut] = "done"

    def flush_expected(self, trace, n, where):
        """The first n records are the finishes of the n oldest pending steps, and no finish follows."""
        calls = [t for t in trace if "call" in t]
        for t in calls[:n]:
            assert t["call"] == "arctopk_exchange_finish", f"{where}: {n} pending steps are finished first"
            self.finish(t, where)
        assert not [t for t in calls[n:] if t["call"] == "arctopk_exchange_finish"], f"{where}: a finish nobody asked for"
        done = [id(t) for t in calls[:n]]  # (registrations: once per plan, and they may come before the finishes)
        return [t for t in trace if id(t) not in done and "op" not in t and "synchronize" not in t]

    # ---- one hook call -----------------------------------------------------------------------------
    def hook(self, b, last, step, where):
        o, trace, ws = self.o, step["trace"], self.ws
        shapes = R.BUCKETS[b]
        numel = bucket_numel(shapes)
        nbytes = numel * self.esz
        path = self.path(b)
        fut = len(self.futs)
        self.futs.append("done")
        if path == "ValueError":  # refused before anything is called or changed
            assert trace == [{"raised": "ValueError"}], where
            self.futs[fut] = "lost"
            return
        comms = ws > 1 or o["force_exchange"]
        efc = N.EF_CODE[self.ef]
        dense = path in ("warmup", "ef21-first")
        # every path but the step finishes what is pending first: collectives of torch's group and of the
        # exchange are never in flight together, and a phase-by-phase call decodes in call order
        same = any(e.b == b or e.stream != self.stream for e in self.pend)
        trail_flush = self.trail is not None and path != "step"
        nflush = len(self.pend) if (path not in ("step", "w16step") or same or trail_flush) else 0
        if dense:
            rest = self.flush_expected(trace, nflush, where)
            coll = dict(coll="all_reduce", dtype="f32" if self.f32 else "bf16", numel=numel, buf="bucket",
                        async_op=path == "warmup")
            assert rest == [coll], where
            self.bits += (2 * (ws - 1) if path == "warmup" else 1) * numel * self.esz * 8
            if path == "ef21-first":
                self.residual.add(b)
            self.iter += int(last)
            return
        # a compressed call: its seed, the observed bucket order, the projections claimed
        seed = int(torch.randint(0, 1_000_000_000, (1,), generator=self.seeds))
        self.nseed = int(torch.randint(0, 1_000_000_000, (1,), generator=self.seeds.clone_state()))
        err_in = int(self.ef != "ef14" or b in self.residual)
        if self.ef != "noef":
            self.residual.add(b)
        if self.last_b is not None and self.last_b != b:
            self.succ[self.last_b] = b
        self.last_b = b
        self.planned.add(b)
        zr = b in self.zr and self.ef == "ef14" and o["err_zero_rows"]
        self.zr.discard(b)
        device_v = o["projections"] == "device"
        E = "NULL" if self.ef == "noef" else "error_dict[b]"
        gE = "global_error_dict[b]" if self.ef == "ef21" else "NULL"
        plan = f"plan[{b}]"
        ratio = R.RATIO
        if self.c4:  # the ramp: 0.8 down to the ratio over 100 iterations, a plan of its own per ratio --
            ratio = 0.8 - (0.8 - R.RATIO) * (self.iter / 100)  # nothing of the previous plan is vouched for
            self.zr.discard(b), self.v_drawn.pop(b, None), self.bound.pop(b, None)
            zr = False
        bits = plan_bits(shapes, self.esz * 8, self.c4, path in ("wire16", "w16step"), ratio)

        def claim():
            draw = self.v_drawn.pop(b, None) != seed
            self.v_stream[b] = self.stream
            return draw

        if path in PHASED:
            enc, pack, dec, swire, pwire, pbuf = PHASED[path]
            rest = self.flush_expected(trace, nflush, where)
            draw = claim() if device_v else False
            want = [] if device_v else ["host_projections"]
            want += ["arctopk_draw_projections"] * draw + [enc] + ["projection_consumed"] * (not device_v)
            want += ["arctopk_comm_allreduce"] * comms + ["select", pack] + ["arctopk_comm_allreduce"] * comms + [dec]
            got = [t.get("call") or t.get("plan_call") or next(iter(t)) for t in rest]
            assert got == want, f"{where}: {got}"
            for t in rest:
                assert t.get("stream", "caller") == self.stream and t.get("plan", plan) == plan, f"{where}: {t}"
                assert "unknown" not in t.values(), f"{where}: {t}"
            ars = [t for t in rest if t.get("call") == "arctopk_comm_allreduce"]
            if comms:
                assert [(t["comm"], t["buf"], t["dtype"]) for t in ars] == [("sk", "sketch", swire), ("pk", pbuf, pwire)], where
            by = {(t.get("call") or t.get("plan_call")): t for t in rest}
            assert by["select"]["world_size"] == ws and by["select"]["next"] == "NULL", where
            if path == "wire16":
                assert (by[enc]["err_in"], by[pack]["err_in"], by[pack]["ef"], by[dec]["ef"]) == (err_in, err_in, efc, efc), where
                assert (by[pack]["packed_bf16"], by[dec]["packed_bf16"], by[dec]["out"]) == ("packed16", "packed16", "bucket"), where
                assert (by[pack]["err"], by[dec]["gerr"]) == (E, gE), where
                self.count["wire16_calls"] += 1
            else:
                if path == "mixed":  # zero rows are never claimed: a selected row keeps its rounding remainder
                    assert (by[enc]["err_in"], by[pack]["err_in"]) == (err_in, err_in), where
                    assert (by[dec]["ef"], by[dec]["gerr"], by[dec]["out"]) == (N.EF14, "NULL", "bucket"), where
                else:
                    assert (by[dec]["gerr_f32"], by[dec]["out_bf16"], by[dec]["world_size"]) == (gE, "bucket", ws), where
                assert (by[enc]["grad_bf16"], by[enc]["err_f32"], by[pack]["err_f32"]) == ("bucket", E, E), where
                self.count["mixed_calls"] += 1
            self.bits += 2 * (ws - 1) * bits
            self.iter += int(last)
            return
        if path == "host_staged":
            rest = [t for t in self.flush_expected(trace, nflush, where) if "event" not in t]
            draw = claim() if device_v else False
            nxt = self.predraw(b) if device_v else None
            want = [] if device_v else ["host_projections"]
            want += ["arctopk_draw_projections"] * draw + ["encode"] + ["projection_consumed"] * (not device_v)
            want += ["all_reduce"] * (ws > 1) + ["select", "pack", "stage_through_host"] + ["all_reduce"] * (ws > 1) + ["decode"]
            got = [t.get("call") or t.get("plan_call") or t.get("coll") or next(iter(t)) for t in rest]
            assert got == want, f"{where}: {got}"
            by = {(t.get("call") or t.get("plan_call")): t for t in rest}
            assert (by["encode"]["err_in"], by["encode"]["err"], by["decode"]["gerr"]) == (err_in, E, gE), where
            assert (by["select"]["next"], by["select"]["next_seed"]) == ((f"plan[{nxt}]", self.nseed) if nxt is not None else ("NULL", 0)), where
            if nxt is not None:
                self.v_drawn[nxt], self.v_stream[nxt] = self.nseed, self.stream
            if o["phase_events"] is not None:  # every phase marked on the caller's stream
                assert len([t for t in trace if "event" in t and t["stream"] == self.stream]) == 9, where
            self.bits += 2 * (ws - 1) * bits
            self.iter += int(last)
            return

        # ---- the one-native-call step -------------------------------------------------------------
        w16 = path == "w16step"
        if w16:
            zr = False  # ... nor on the bf16 wire
        dd = bool(o["defer_decode"])  # (None: DDP's own buckets only, and the rig's are synthetic)
        defer = dd and o["async_exchange"] and not last
        marked = o["phase_events"] is not None
        draw = claim() if device_v else False
        nxt = self.predraw(b) if device_v else None
        calls = [t for t in trace if "call" in t and t["call"] != "arctopk_exchange_finish"]
        sel_backward = o["select_streams"] == "on" or (
            o["select_streams"] == "auto" and self.sel_small_last >= o["select_stream_min_buckets"])
        # a trailing step: world size 1 without collectives, a deferring caller, no markers, device
        # projections, not EF21, none recorded yet, no select-stream backward, not the bf16 wire, a small bucket
        may_trail = (not comms and defer and not marked and device_v and o["trail_bytes"] > 0 and self.ef != "ef21"
                     and self.trail is None and not sel_backward and not w16 and nbytes <= o["trail_bytes"])
        if may_trail:
            assert not nflush and trace[0].get("call") == "arctopk_exchange_trail", f"{where}: the bucket may trail"
            t = trace[0]
            assert t == dict(call="arctopk_exchange_trail", plan=plan, bucket="bucket", err=E, gerr=gE, ef=efc, err_in=err_in,
                             draw=int(draw), seed=seed, V="NULL", stream=self.stream), f"{where}: {t}"
            status = self.status.pop(0) if self.status else 0
            if status == 0:  # recorded: nothing else is called; carried by the next step
                assert len(trace) == 1, where
                self.trail = Entry(plan, b, self.stream, "NULL", fut)
                self.pend.append(self.trail)
                self.futs[fut] = self.trail
                self.count["trail_calls"] += 1
                self.sel_small += int(nbytes <= o["select_stream_bytes"])
                self.bits += 2 * (ws - 1) * bits
                self.iter += int(last)
                return
            if status != N.EINVAL:  # (EINVAL: not a bucket of single-block selects; the step runs)
                assert trace[1:] == [{"raised": "RuntimeError"}], where
                self.futs[fut] = "lost"
                return
            trace = trace[1:]
        else:
            assert not [t for t in calls if t["call"] == "arctopk_exchange_trail"], f"{where}: the bucket may not trail"
        # a recorded trail: carried by this step, unless its stream differs, it is this plan's, or this is a bf16-wire step
        carried = None
        if self.trail is not None and not (self.trail.stream != self.stream or self.trail.b == b or w16):
            carried = self.trail
            self.pend.remove(carried)
            self.trail = None
            nflush = len(self.pend) if any(e.b == b or e.stream != self.stream for e in self.pend) else 0
        rest = self.flush_expected(trace, nflush, where)
        grouped = (comms and o["async_exchange"] and not marked and o["exchange_groups"] != "off" and not w16
                   and (o["exchange_groups"] == "all" or not self.pend or last))
        units = R.GROUPS[3 if b == 1 else 2] if grouped else ((0, 0),)
        if w16 != self.bound.get(b, False):  # bound between the plan's steps only
            assert rest[0] == dict(call="arctopk_plan_bind_wire16", plan=plan, packed_bf16="packed16" if w16 else "NULL"), where
            rest = rest[1:]
            self.bound[b] = w16
        small = nbytes <= o["select_stream_bytes"]
        self.sel_small += int(small)
        if last:
            self.sel_small_last, self.sel_small = self.sel_small, 0
        side = "NULL"
        if (o["select_streams"] != "off" and not grouped and not marked and dd and not w16
                and (o["select_streams"] == "on" or (small and self.sel_small_last >= o["select_stream_min_buckets"]))):
            self.sel_turn ^= 1  # the two select streams alternate
            side = f"sel{self.sel_turn}"
            nxt = None  # the select does not draw the next call's V
        depth = 2 if (comms or side != "NULL") else 1
        marks = "NULL"
        if marked:
            marks, self.nmarks = f"marks[{self.nmarks}]", self.nmarks + 1
        if not device_v:
            assert rest[0].get("host_projections") == plan, where
            assert rest[-1].get("plan_call") == "projection_consumed", where
            rest = rest[1:-1]
        assert len(rest) >= len(units), f"{where}: {len(units)} steps expected: {rest}"
        for ui, ((off, v_off), t) in enumerate(zip(units, rest)):
            last_u = ui == len(units) - 1
            u_defer = defer if last_u else True  # a group's decode is finished by a later one
            ride = self.pend.pop(0) if len(self.pend) >= depth else None
            if carried is not None and ui == 0:
                self.pend.append(carried)
            fin = [] if u_defer else self.pend[:]
            if not u_defer:
                del self.pend[:]
            plus = f"+{off * self.esz}" if off else ""
            if grouped:
                u_draw = int(draw and ui == 0) if device_v else 0
                u_next = (f"plan[{b}].group[{ui + 1}]", seed) if (device_v and draw and not last_u) else ("NULL", 0)
            else:
                u_draw, u_next = int(draw), ("NULL", 0)
            if last_u and nxt is not None:
                u_next = (f"plan[{nxt}]", self.nseed)
            want = dict(call="arctopk_exchange_step", plan=f"plan[{b}].group[{ui}]" if grouped else plan,
                        bucket="bucket" + plus, err="NULL" if E == "NULL" else E + plus, gerr="NULL" if gE == "NULL" else gE + plus,
                        ef=efc, err_in=N.ERR_IN_ZERO_ROWS if (zr and err_in and not grouped) else err_in, draw=u_draw,
                        seed=seed, next=u_next[0], next_seed=u_next[1], sketch_comm="sk" if comms else "NULL",
                        packed_comm="pk" if comms else "NULL", stream=self.stream, ar_stream="ar" if comms else "NULL",
                        defer=int(u_defer), ride=ride.plan if ride else "NULL", ride_marks=ride.marks if ride else "NULL",
                        finish=[e.plan for e in fin] or "NULL", finish_marks=[e.marks for e in fin] or "NULL", nfinish=len(fin),
                        V="NULL" if device_v else "V" + (f"+{v_off * self.esz}" if v_off else ""), marks=marks, sel_stream=side,
                        trail=carried.plan if (carried is not None and ui == 0) else "NULL")
            assert t == want, f"{where}: unit {ui}: " + str({k: (t.get(k), v) for k, v in want.items() if t.get(k) != v})
            status = self.status.pop(0) if self.status else 0
            if status:  # the step failed: RuntimeError; what rode or was to be finished is lost to the FIFO
                tail = [x for x in rest[ui + 1:]]
                assert tail[-1] == {"raised": "RuntimeError"}, where
                for e in ([ride] if ride else []) + fin:
                    if e.fut is not None:
                        self.futs[e.fut] = "stuck"  # (never completed: the caller got the exception)
                self.futs[fut] = "lost"
                return
            for e in ([ride] if ride else []) + fin:  # their decodes are enqueued now
                if e.fut is not None:
                    self.futs[e.fut] = "done"
            if u_defer:
                e = Entry(want["plan"], b, self.stream, marks, fut if last_u else None)
                self.pend.append(e)
                if last_u:
                    self.futs[fut] = e
        assert len(rest) == len(units), f"{where}: more than the {len(units)} steps: {rest[len(units):]}"
        if nxt is not None:
            self.v_drawn[nxt], self.v_stream[nxt] = self.nseed, self.stream
        if self.ef == "ef14" and not grouped and not w16:
            self.zr.add(b)
        if w16:
            self.count["wire16_step_calls"] += 1
            self.count["wire16_calls"] += 1
        self.bits += 2 * (ws - 1) * bits
        self.iter += int(last)

    def predraw(self, b):
        """The bucket whose V this call's select draws: the one that followed b last time, if its plan
        exists and V_ring[0] of it was last used on this stream."""
        nb = self.succ.get(b)
        if nb is None or nb not in self.planned or self.v_stream.get(nb, self.stream) != self.stream:
            return None
        return nb

    # ---- a case ------------------------------------------------------------------------------------
    def run(self, steps, script):
        self.status = []
        it = iter(steps)
        for s in script:
            if s[0] == "stream":
                self.stream = R.STREAMS[s[1]]
            elif s[0] == "status":
                self.status = list(s[2])
            elif s[0] == "set":
                self.o[s[1]] = s[2]
            else:
                step = next(it)
                n = steps.index(step)
                where = f"{self.cid} step {n} {s}"
                if s[0] == "wait":  # flush_exchange(upto=): in call order, up to and including that Future's step
                    e = self.futs[s[1]]
                    k = self.pend.index(e) + 1 if isinstance(e, Entry) and e in self.pend else 0
                    assert self.flush_expected(step["trace"], k, where) == [], where
                else:
                    self.hook(s[1], len(s) > 2 and s[2], step, where)
                self.check_state(step["state"], where)
                for t in step["trace"]:
                    assert "unknown" not in [v for v in t.values() if isinstance(v, str)], f"{where}: {t}"

    def check_state(self, snap, where):
        assert snap["pend"] == [e.plan for e in self.pend], where
        assert snap["trail"] == (self.trail.plan if self.trail else None), where
        # a Future is done exactly when its step's decode is enqueued: at once when nothing is deferred
        done = [f == "done" for f in self.futs if f != "lost"]
        assert snap["futures_done"] == done, f"{where}: {snap['futures_done']} {self.futs}"
        assert snap["iter"] == self.iter and snap["comm_bits_this_round"] == self.bits, (where, self.bits)
        for k, v in self.count.items():
            assert snap[k] == v, f"{where}: {k}"
        assert (snap["sel_small"], snap["sel_small_last"], snap["sel_turn"]) == (
            self.sel_small, self.sel_small_last, self.sel_turn), where
        assert sorted(int(b) for b, ok in snap["zero_rows"].items() if ok) == sorted(self.zr), where
        res = "f32" if self.f32 or self.o["error_dtype"] is not None or self.o["ef21_error_dtype"] is not None else "bf16"
        if self.ef == "ef21" and self.o["ef21_error_dtype"] is None:
            res = "f32" if self.f32 else "bf16"
        if self.ef == "ef14" and self.o["error_dtype"] is None:
            res = "f32" if self.f32 else "bf16"
        assert snap["error_dtype"] == {b: res for b in sorted(self.residual)}, where
        assert snap["global_error_dtype"] == ({b: res for b in sorted(self.residual)} if self.ef == "ef21" else {}), where
        assert {int(b) for b, v in snap["wire16_bound"].items() if v} == {b for b, v in self.bound.items() if v}, where


@pytest.mark.parametrize("cid,case", MATRIX, ids=[cid for cid, _ in MATRIX])
def test_matrix(cid, case):
    steps = R.run_case(**case)
    script = case.get("script") or R.BACKWARD * (3 if case.get("ef") == "ef21" else 2)
    model = Model(cid, **case)
    model.run(steps, script)
    assert len(steps) == len([s for s in script if s[0] in ("hook", "wait")])
    if script[-1][0] == "hook" and len(script[-1]) > 2 and steps[-1]["trace"][-1:] != [{"raised": "ValueError"}]:
        # the backward's last bucket finishes everything: nothing pending, every Future done
        assert steps[-1]["state"]["pend"] == [] and all(steps[-1]["state"]["futures_done"][-1:]), cid


def test_the_matrix_covers_what_it_claims():
    """Both values of draw, next and defer, rides at both depths, grouped, side-stream and trailing steps,
    flushes and failures all occur in the matrix (a rule that never applies checks nothing)."""
    seen = set()
    for cid, case in MATRIX:
        for step in R.run_case(**case):
            for t in step["trace"]:
                if t.get("call") == "arctopk_exchange_step":
                    seen |= {("draw", t["draw"]), ("next", t["next"] != "NULL"), ("defer", t["defer"]),
                             ("ride", t["ride"] != "NULL", t["sketch_comm"] != "NULL"), ("group", ".group[" in t["plan"]),
                             ("side", t["sel_stream"]), ("trail", t["trail"] != "NULL"), ("err_in", t["err_in"]),
                             ("V", t["V"].split("+")[0]), ("marks", t["marks"] != "NULL")}
                seen.add(t.get("call") or t.get("raised") or t.get("coll"))
    for want in [("draw", 0), ("draw", 1), ("next", True), ("next", False), ("defer", 0), ("defer", 1),
                 ("ride", True, False), ("ride", True, True), ("group", True), ("side", "sel0"), ("side", "sel1"),
                 ("trail", True), ("err_in", 0), ("err_in", 1), ("err_in", 2), ("V", "V"), ("V", "NULL"), ("marks", True),
                 "arctopk_exchange_finish", "arctopk_exchange_trail", "arctopk_plan_bind_wire16",
                 "RuntimeError", "ValueError", "all_reduce"]:
        assert want in seen, want


if __name__ == "__main__":
    for cid, kw in MATRIX:
        for i, step in enumerate(R.run_case(**kw)):
            print(json.dumps({"case": cid, "n": i, **step}, sort_keys=True, default=str))
