/*
 * arctopk.h -- C ABI of libarctopk.so, the MI355X (gfx950) ARC-TopK / TopK /
 * RandK gradient-bucket codec.
 *
 * Boundary.  The reference (Aris-ma/AllreduceTopK) is pure Python: its hot path
 * is the DDP comm hook `group_topk_hook(state, bucket)`
 * (comm_hooks/group_topk_hook_no_reshape.py:190-297) plus the TopK/RandK hook
 * `sparse_hook_sync` (comm_hooks/sparse_hook.py:163-304), and all arithmetic in
 * them is torch aten ops.  This library replaces exactly those aten op sequences
 * with stream-ordered HIP kernels; the collectives stay with the caller
 * (torch.distributed / RCCL), so the drop-in Python hooks in
 * allreducetopk_amd/comm_hooks/ call, per bucket:
 *
 *     arctopk_encode  -> all_reduce(sketch) -> arctopk_select -> arctopk_pack
 *                     -> all_reduce(packed) -> arctopk_decode
 *
 * Conventions.
 *  - Every entry point returns 0 on success or a nonzero status (a hipError_t
 *    value, or one of the ARCTOPK_E* codes below).  Nothing throws across the ABI.
 *  - Device pointers are plain element pointers into device memory; `stream` is
 *    a hipStream_t passed as void*.  Compute entry points only enqueue work on
 *    `stream`: no host synchronisation, no allocation (graph-capturable).
 *  - A plan owns its device tables and a select workspace; calls that share a
 *    plan must be ordered on one stream.
 *  - Element types: ARCTOPK_F32 (every BASELINE config's bucket) and ARCTOPK_BF16
 *    (the Llama driver's default dtype).  Bucket-typed buffers are passed as void*.
 *    The TopK / RandK entry points are fp32 only.
 */
#ifndef ARCTOPK_H
#define ARCTOPK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes besides hipError_t */
#define ARCTOPK_OK 0
#define ARCTOPK_EINVAL 1001     /* bad argument (null pointer, ratio out of (0,1], r out of range) */
#define ARCTOPK_ERESHAPE 1002   /* ND tensor numel not divisible by m = 2*t^2 (ref :76 raises) */
#define ARCTOPK_EDTYPE 1003     /* unsupported element type */
#define ARCTOPK_EEMPTY 1004     /* empty tensor: torch.topk(k=1) on 0 elements raises */
#define ARCTOPK_ENOCOMM 1005    /* the RCCL library could not be loaded / lacks entry points */
#define ARCTOPK_ETIMEOUT 1006   /* a communicator's collective (or its creation) outlived the
                                   process group's timeout; the communicator was aborted */
#define ARCTOPK_EABORTED 1007   /* the communicator was aborted (by arctopk_comm_abort, or after
                                   an error of another communicator of this process) */
#define ARCTOPK_ECOMM 1100      /* RCCL error: ARCTOPK_ECOMM + ncclResult_t */

/* error-feedback modes (ref GroupTopKState.use_error_feedback, :149, :224-250) */
#define ARCTOPK_EF_NONE 0
#define ARCTOPK_EF14 1
#define ARCTOPK_EF21 2
/* err_in of the EF14 entry points: 0 the residual is all zeros and is not read (the first call),
 * 1 it is read, 2 it is read except the rows the plan's last select chose (arctopk_encode) */
#define ARCTOPK_ERR_IN_NONE 0
#define ARCTOPK_ERR_IN_READ 1
#define ARCTOPK_ERR_IN_ZERO_ROWS 2

/* element types of a bucket (and of its sketch, projections and packed values, which
 * the reference keeps in the bucket's dtype: group_topk_hook_no_reshape.py:49, :263) */
#define ARCTOPK_F32 0
#define ARCTOPK_BF16 1   /* bfloat16 storage; arithmetic in fp32, each value the reference
                            rounds to bf16 rounded the same way (round-to-nearest-even) */

/* segment kinds */
#define ARCTOPK_SEG_RAW 0     /* 1-D tensor: the "sketch" is the tensor itself (ref :19-41) */
#define ARCTOPK_SEG_SKETCH 1  /* 2-D [n,m] or ND reshaped to [d/m, m], m = 2*t^2 (ref :44-102) */
#define ARCTOPK_SEG_DENSE 2   /* 1-D tensor of a plan with ARCTOPK_PLAN_DENSE_1D: not compressed -- no
                                 sketch, no select, every element ("row", m = 1) selected
                                 (group_topk_hook_no_reshape_c4.py:19-25) */

/* plan flags (arctopk_plan_create_ex): the reference's c4 variant of the hook
 * (comm_hooks/group_topk_hook_no_reshape_c4.py) */
#define ARCTOPK_PLAN_DENSE_1D 1       /* 1-D tensors are DENSE segments instead of RAW ones */
#define ARCTOPK_PLAN_RESTART_DRAWS 2  /* device projections: every SKETCH tensor's V is drawn from
                                         Philox offset 0 of the call's seed (a fresh generator per
                                         tensor, c4 :31-39, :70-77) instead of one advancing stream */

typedef struct arctopk_plan arctopk_plan;

/* Totals of a plan, for sizing the caller's buffers. */
typedef struct {
    int64_t numel;       /* bucket elements (bucket.buffer().numel())                  */
    int64_t sketch_len;  /* floats of the concatenated sketch: sum n*r (SKETCH) + d (RAW);
                            DENSE segments add nothing (0: no sketch all-reduce, no select)  */
    int64_t v_len;       /* floats of the concatenated projections: sum m*r over SKETCH   */
    int64_t packed_len;  /* floats of the packed buffer: every segment's k_rows*m values,
                            each segment starting 16-B aligned (<= 3 pad floats between)  */
    int64_t sel_rows;    /* sum of selected rows (length of the row list)                 */
    int64_t rows_total;  /* sum n (length of the slot map)                                */
    int32_t nseg;        /* gradient views in the bucket                                  */
    int32_t r;           /* sketch rank                                                   */
    int64_t values_len;  /* sum_k: selected elements (ref values_memory length, :261-263)  */
} arctopk_plan_info;

/* Per-segment geometry (for the host-side mirror and tests). */
typedef struct {
    int64_t offset;      /* element offset in the bucket                 */
    int64_t n, m;        /* rows, columns (m = 1 for RAW)                 */
    int64_t k_rows;      /* selected rows: max(1, int(n * ratio))  (ref cal_k :173-187); DENSE: n */
    int64_t sketch_off;  /* float offset in the sketch buffer            */
    int64_t v_off;       /* float offset in the projection buffer (-1: RAW, DENSE) */
    int64_t packed_off;  /* element offset in the packed buffer          */
    int64_t row_off;     /* offset in the slot map (global row index)    */
    int64_t sel_off;     /* offset in the selected-row list              */
    int32_t kind;        /* ARCTOPK_SEG_RAW / ARCTOPK_SEG_SKETCH / ARCTOPK_SEG_DENSE */
    int32_t pad;
} arctopk_segment;

/*
 * Build the plan of one bucket layout.  `dims` holds the shapes of
 * bucket.gradients() concatenated, `ndims[i]` the rank of tensor i.  Geometry and
 * k follow the reference: 1-D -> RAW; 2-D -> [shape0, shape1]; ND -> [d/m, m]
 * with m = 2*shape[-1]^2 (group_topk_hook_no_reshape.py:16-102, cal_k :173-187).
 * Replaces: the per-call Python loop over bucket.gradients() (:111-129, :259).
 */
int arctopk_plan_create(const int64_t* dims, const int32_t* ndims, int32_t ntensors, int32_t r,
                        double compress_ratio, int32_t dtype, int32_t device, arctopk_plan** out);
/*
 * arctopk_plan_create with plan flags (ARCTOPK_PLAN_*; 0: arctopk_plan_create).  With
 * ARCTOPK_PLAN_DENSE_1D a 1-D tensor is a DENSE segment: n = numel, m = 1, k_rows = n, v_off = -1;
 * it adds nothing to sketch_len and n to values_len / packed_len / sel_rows / rows_total.  It
 * has no encode work: arctopk_encode leaves its range of E untouched, and EF14's X = G + E
 * (err_in of the plan's last arctopk_encode; else X = G) is formed by the pack, which therefore
 * needs `grad` for EF14 too.  The select leaves the identity in its row list and slot map ranges
 * (written once per binding of the plan's buffers, and by every select on other buffers); pack
 * and decode stream it straight through, every element selected, without reading either:
 *   NONE : packed = G                          out = mean(packed)
 *   EF14 : packed = G + E, E := 0              out = mean(packed)
 *   EF21 : D = G - E; packed = D; E += D       out = gE + mean(packed); gE := out
 * Replaces: the c4 hook's 1-D branch (group_topk_hook_no_reshape_c4.py:19-25, cal_k :206-207).
 */
int arctopk_plan_create_ex(const int64_t* dims, const int32_t* ndims, int32_t ntensors, int32_t r,
                           double compress_ratio, int32_t dtype, int32_t device, int32_t flags,
                           arctopk_plan** out);
int arctopk_plan_destroy(arctopk_plan* plan);
/* Host-only: the geometry a plan would have (no device memory touched); segs_out may be NULL. */
int arctopk_plan_describe(const int64_t* dims, const int32_t* ndims, int32_t ntensors, int32_t r,
                          double compress_ratio, arctopk_segment* segs_out, arctopk_plan_info* info);
int arctopk_plan_describe_ex(const int64_t* dims, const int32_t* ndims, int32_t ntensors, int32_t r,
                             double compress_ratio, int32_t flags, arctopk_segment* segs_out,
                             arctopk_plan_info* info);
int arctopk_plan_query(const arctopk_plan* plan, arctopk_plan_info* info);
/*
 * A plan over the consecutive segments [seg_begin, seg_end) of `parent` (a group of the bucket's
 * tensors): the exchange pipeline's unit below a bucket.  Geometry, k and
 * projections (the parent's Philox offsets) are the parent's; every offset is relative to the
 * group's first segment, so bind the group to the parent's buffers at those segment's offsets
 * (sketch_off, row_off, row_off, packed_off, first SKETCH v_off) and pass bucket / residual
 * pointers at its element offset.  The group inherits the parent's plan flags.  ARCTOPK_EINVAL when the group's base offsets are not
 * multiples of 8 elements (sketch, packed, bucket, V) and 4 (slot map), which keeps every vector
 * path of the kernels aligned as in the parent.  Destroy with arctopk_plan_destroy.
 * Replaces: nothing in the reference (its per-tensor sketch all-reduce, :33, :58, :88, is the
 * finest grain; the group is a run of those tensors).
 */
int arctopk_plan_group(const arctopk_plan* parent, int32_t seg_begin, int32_t seg_end,
                       arctopk_plan** out);

int arctopk_plan_segment(const arctopk_plan* plan, int32_t i, arctopk_segment* seg);

/*
 * K1 encode.  EF pre-apply fused with the rank-r sketch of every tensor.
 *   ef = NONE : X = G
 *   ef = EF14 : X = G + E (err_in = 1) or X = G (first call, err_in = 0); writes E := X
 *               err_in = 2 (ARCTOPK_ERR_IN_ZERO_ROWS): as 1, and the caller states that `err` has not
 *               been written since this plan's last EF14 pack or fused finalize (arctopk_pack,
 *               arctopk_step, arctopk_exchange_step / _finish on the plan's bound buffers), which
 *               left every row its select chose all zeros.  The library keeps its own record of that
 *               pack or finalize: the residual pointer and the stream it was enqueued on, dropped by
 *               anything else that writes the bound row list or slot map (arctopk_select,
 *               arctopk_select_draw, arctopk_plan_bind, a step in another EF mode, a failed step).
 *               Only if the record holds for `err`, and `stream` is that stream or one the library
 *               made wait for it, the wave-per-row tiles (rows of >= 64 elements, r = 4) read the
 *               bound slot map and issue no loads from E for the rows it marks (slot >= 0); X, E and
 *               the sketch are bit for bit those of err_in = 1.  Otherwise, and for every other tile
 *               kind, rank, carried trailing step and the sparse entry points, 2 means 1.
 *   ef = EF21 : X = G - E (nothing written but the sketch)
 * sketch[SKETCH seg] = X.view(n,m) @ V  ([n][r] row-major); sketch[RAW seg] = X.
 * `V` is the concatenation of each SKETCH tensor's [m][r] projection in bucket order.
 * Replaces: input_tensor.add_(error, alpha=+-1) (:227, :234), tensor @ V (:53, :83),
 *           P = P_local.clone() (:31, :56, :86).
 */
int arctopk_encode(const arctopk_plan* plan, const void* grad, void* err, int32_t ef,
                   int32_t err_in, const void* V, void* sketch, void* stream);

/*
 * K2 select.  From the all-reduced sketch: P /= world_size, row energy
 * sum_j P[row][j]^2 or P^2 (RAW), top-k_rows rows per segment.  The sum is
 * sequential in j, ((q0 + q1) + q2) + ..., in fp32 (bf16: bf16 squares, the sum
 * rounded once): the bits of torch's CPU sum over dim 1 for r <= 4 in both
 * dtypes and for fp32 r = 8.  torch adds in another order for fp32 r = 5, 6, 7
 * (last bits, at most 2 (r - 1) 2^-24 relative) and for bf16 r = 5 .. 8 (one
 * bf16 step, on the rare row whose sum lies at a rounding boundary).  Ties at the k-th energy: lowest rows
 * first.  Writes the selected rows ascending (rowlist[sel_off ..]) and, for every
 * row, its packed slot or -1 (slotmap[row_off + row]).
 * Replaces: P /= ws; norms = sum(P**2, 1); torch.topk(norms, k, sorted=False);
 *           row*m + arange(m) index materialisation (:34-38, :59-66, :89-96).
 */
int arctopk_select(const arctopk_plan* plan, const void* sketch, int32_t world_size,
                   int32_t* rowlist, int32_t* slotmap, void* stream);

/*
 * arctopk_select, and in the same launch (its trailing blocks, which run beside the
 * latency-bound select blocks) the device projections of the NEXT call: V_next =
 * arctopk_draw_projections(next, next_seed).  The caller predicts the next call (plan and
 * seed) and keeps V_next only when that call's seed matches; otherwise it draws again.
 * `next` must have `plan`'s dtype and device; `next` = NULL is arctopk_select.
 * Removes the draw launch (and its kernel boundary) from the next call's critical path.
 */
int arctopk_select_draw(const arctopk_plan* plan, const void* sketch, int32_t world_size,
                        int32_t* rowlist, int32_t* slotmap, const arctopk_plan* next,
                        uint64_t next_seed, void* next_V, void* stream);

/*
 * Phase markers of a step (arctopk_step / arctopk_exchange_step): `marks` is NULL or an array
 * of ARCTOPK_NMARKS hipEvent_t handles; every non-NULL entry is recorded at that point (for
 * per-phase timing; each record between two kernels idles the GPU a few microseconds).
 * PACKED_AR and DECODE are recorded on the stream that runs them (the exchange stream when
 * there is one).
 */
#define ARCTOPK_MARK_START 0      /* before the projection draw                       */
#define ARCTOPK_MARK_DRAW 1       /* after the draw, before the encode                */
#define ARCTOPK_MARK_ENCODE 2
#define ARCTOPK_MARK_SKETCH_AR 3  /* exchange step only                               */
#define ARCTOPK_MARK_SELECT 4
#define ARCTOPK_MARK_PACK 5
#define ARCTOPK_MARK_PACKED_AR 6  /* exchange step only                               */
#define ARCTOPK_MARK_DECODE 7
#define ARCTOPK_NMARKS 8

/*
 * One-call step at world size 1, where both all-reduces of the hook are identities
 * (group_topk_hook_no_reshape.py:264, :280): [draw V for `seed` when draw != 0] -> encode
 * -> select (+ the next call's projections: next / next_seed, as arctopk_select_draw) ->
 * pack -> decode into `bucket`, on the buffers bound to the plan by arctopk_plan_bind (the
 * sketch, row list, slot map, packed values and projection buffer the phase entry points
 * take as arguments).  One foreign-function call per hook call instead of one per phase.
 * err_in (EF14): 0, 1 or 2 (ARCTOPK_ERR_IN_ZERO_ROWS) with the meaning and the conditions given at
 * arctopk_encode; the step's own pack is what sets the plan's zero-rows record for the next call.
 */
int arctopk_plan_bind(arctopk_plan* plan, void* sketch, int32_t* rowlist, int32_t* slotmap,
                      void* packed, void* V);
int arctopk_step(const arctopk_plan* plan, void* bucket, void* err, void* gerr, int32_t ef,
                 int32_t err_in, int32_t draw, uint64_t seed, const arctopk_plan* next,
                 uint64_t next_seed, void* stream, void* const* marks);

/* ---- the exchange: collectives of the hook (group_topk_hook_no_reshape.py:58, :280) ---- */
/*
 * A communicator for the hook's SUM all-reduces: an RCCL communicator owned by this library
 * (RCCL loaded at run time from `rccl_path`, normally the librccl.so torch itself loaded, so
 * the process holds one RCCL), or a callback (`fn(ctx, buf, count, dtype, stream)` must
 * all-reduce `count` elements at `buf` in place, ordered on `stream`; returns 0 or nonzero).
 * Creating an RCCL communicator is collective: every rank calls arctopk_comm_init_rccl with
 * the id rank 0 obtained from arctopk_comm_unique_id (128 bytes), and it blocks until all have.
 */
typedef struct arctopk_comm arctopk_comm;
typedef int (*arctopk_allreduce_fn)(void* ctx, void* buf, int64_t count, int32_t dtype, void* stream);
int arctopk_comm_unique_id(const char* rccl_path, void* id_out);
int arctopk_comm_init_rccl(const char* rccl_path, const void* id, int32_t nranks, int32_t rank,
                           int32_t device, arctopk_comm** out);
/*
 * Failure detection (the reference's collectives run on ProcessGroupNCCL, whose watchdog turns
 * a hung or failed collective into an error after the group's timeout: cifar10/run_cifar10.py:
 * 55-58).  arctopk_comm_init_rccl_timeout creates the communicator non-blocking
 * (ncclCommInitRankConfig, blocking = 0) and gives up after `timeout_ms` (aborting it:
 * ARCTOPK_ETIMEOUT) when a rank never joins.  With timeout_ms > 0 a watchdog thread of the
 * library then polls ncclCommGetAsyncError and the completion of every collective the
 * exchange step issued on the communicator; an asynchronous RCCL error, or a collective still
 * pending `timeout_ms` after it was enqueued, aborts EVERY RCCL communicator of the library
 * (the GPU kernels of an aborted communicator exit) and leaves the error sticky:
 * arctopk_comm_status returns it, and every later exchange step on the communicator returns
 * it instead of enqueueing work.  Work already queued behind the failed collective (the decode,
 * the caller's copy-back and optimizer step) would then run on partially reduced buffers, so,
 * as ProcessGroupNCCL's async error handling does by default, the watchdog ends the process
 * instead of aborting (stderr message, exit status 1).  ARCTOPK_ASYNC_ERROR_HANDLING (else torch's
 * TORCH_NCCL_ASYNC_ERROR_HANDLING) = 0 or 2 keeps it alive: the error is then raised by the
 * next exchange step.  arctopk_comm_init_rccl = timeout 0: blocking creation, no watchdog.  The
 * device current on the calling thread is left unchanged.
 */
int arctopk_comm_init_rccl_timeout(const char* rccl_path, const void* id, int32_t nranks, int32_t rank,
                                   int32_t device, int64_t timeout_ms, arctopk_comm** out);
int arctopk_comm_status(const arctopk_comm* comm);
int arctopk_comm_abort(arctopk_comm* comm);
int arctopk_comm_init_callback(arctopk_allreduce_fn fn, void* ctx, int32_t nranks, int32_t rank,
                               arctopk_comm** out);
/*
 * Measurement only: an "emulated wire" communicator of world size 1 (results are those of a
 * one-rank all-reduce: the buffer is left unchanged) whose all-reduce costs what an
 * `emul_ranks`-rank ring all-reduce costs the local GPU: a kernel of `blocks` workgroups
 * (RCCL's CU footprint) that reads and rewrites 2 (R - 1) / R of the buffer's bytes in HBM,
 * paced to take at least latency_us + 2 (R - 1) / R * bytes / busbw_gbs.  Lets one GPU measure
 * the exchange step beside an N-rank wire.
 */
int arctopk_comm_init_wire(int32_t emul_ranks, double busbw_gbs, double latency_us, int32_t blocks,
                           int32_t device, arctopk_comm** out);
/* Destroy a communicator.  An RCCL communicator created non-blocking is finalized first
 * (ncclCommFinalize, polled until its pending operations have flushed, at most its timeout;
 * past it, or on an error, it is aborted and ARCTOPK_ETIMEOUT / the RCCL error is returned),
 * then destroyed. */
int arctopk_comm_destroy(arctopk_comm* comm);
int arctopk_comm_size(const arctopk_comm* comm);
/* in-place SUM all-reduce of `count` elements (ARCTOPK_F32 / ARCTOPK_BF16), stream-ordered */
int arctopk_comm_allreduce(arctopk_comm* comm, void* buf, int64_t count, int32_t dtype, void* stream);

/*
 * One bucket call of the hook, collectives included, in one host call.  World size = the
 * communicators' size (both NULL: world size 1, no collectives issued).  On `stream`:
 *   [draw] -> encode -> all_reduce(sketch, sketch_comm) -> select (+ next V)
 *          -> pack -> the `finish` steps' deferred decodes -> [all_reduce(packed) -> decode]
 * defer = 1: this step's decode is deferred to arctopk_exchange_finish(plan, ...) (or to a
 *   later step's `ride` / `finish`); with communicators its packed all-reduce runs on
 *   `ar_stream` after the pack kernel, which completes the event that stream waits for (no
 *   marker packet on `stream`), so the caller's stream encodes the next bucket while these
 *   packed values are on the wire.  defer = 0: the decode follows on `stream`; given an
 *   `ar_stream` (and no markers), the packed all-reduce runs there too and `stream` waits for
 *   it just before the decode, so the `finish` steps' decodes run beside it on the wire;
 *   otherwise the all-reduce is inline on `stream`.
 *   Without communicators (world size 1) and markers the all-reduces are identities: for EF14 /
 *   noef no packed values are formed at all -- the decode (deferred or inline) takes the
 *   selected rows from the residual / the bucket and zeroes the rest, the same bits as pack then
 *   decode; for EF21, defer = 1 defers the pack as well, to the first blocks of the
 *   next step's encode launch (that step's `ride`; same EF mode and dtype, other bucket and
 *   residual buffers) or arctopk_exchange_finish.  Until the decode the plan's packed buffer and
 *   the residual's selected rows are not final.  CONTRACT at world size 1 with defer = 1: the
 *   deferred decode (and EF21's deferred pack) READS `bucket` and `err` -- the selected rows
 *   are taken from them when it runs, not when this step is enqueued -- so a caller must leave
 *   the bucket and residual (and gerr) untouched on every stream until that decode has been
 *   enqueued (by arctopk_exchange_finish or a later step's `ride` / `finish`); the DDP hook does
 *   (the Reducer reads a bucket only after its Future completes, which flushes the decode).
 * ride: an earlier step's deferred decode, run inside this step's select launch (extra blocks of
 *   the single-block select launch, or of the multi-block select's last, fused write launch: the
 *   select's latency then hides behind the decode's HBM stream), else right after the select;
 *   ride_marks are that step's markers.
 * finish[0 .. nfinish): earlier deferred steps decoded after this pack, in order.
 * `V`: the projections to encode with (NULL: the plan's bound projection buffer, drawn there
 * for `seed` when draw != 0).  `marks`: see ARCTOPK_MARK_*.
 * sel_stream (NULL: `stream`): a SELECT STREAM.  The draw, the encode and the sketch all-reduce
 *   stay on `stream`; the select (+ ride), the pack, the `finish` decodes and this step's own
 *   decode go on sel_stream after an event on the encode, so the latency-bound select chain runs
 *   beside the caller's next encode.  A deferred step remembers its select stream: its decode
 *   (arctopk_exchange_finish, or a later step's `ride`) goes there, and the finishing stream then
 *   waits for it; a ride from another select stream is finished on its own instead of riding.
 *   A non-deferred step leaves `stream` waiting for its decode.  With a select stream: `next`
 *   must be NULL (the next call draws its own projections), markers disable it, and with
 *   communicators `ar_stream` must be a third stream (ARCTOPK_EINVAL otherwise).
 * trail (NULL: none): a step recorded by arctopk_exchange_trail.  World size 1 without markers,
 *   when both plans qualify (same dtype, r = 4, EF mode and err_in; EF14 / noef; the trail's tensors
 *   all single-block selects and no column-split encode, this plan's with a multi-block
 *   select), the trail's encode tiles run as extra blocks of this step's encode launch and its
 *   selects as extra blocks of this step's first compact launch; otherwise it is enqueued on its
 *   own first.  Either way it leaves this call as a deferred step (its decode: a later `ride` /
 *   `finish` / arctopk_exchange_finish, like a defer = 1 step's).
 * err_in (EF14): 0, 1 or 2 (ARCTOPK_ERR_IN_ZERO_ROWS) with the meaning and the conditions given at
 *   arctopk_encode.  The record that 2 relies on is set by this plan's pack (with communicators)
 *   or fused finalize (world size 1), on the stream it is enqueued on; a finalize that rides in a
 *   later step's select on a select stream, a carried trailing step and the groups of a bucket
 *   leave the next encode on the caller's stream to run as 1.
 * A plan bound with arctopk_plan_bind_wire16 runs the step on the bf16 wire: the pack is
 *   arctopk_pack_wire16's (completing the same event), the packed all-reduce moves the bound bf16
 *   buffer as ARCTOPK_BF16 under the same rules, and the decode is arctopk_decode_wire16's -- by
 *   arctopk_exchange_finish when deferred, a separate launch after the select when the plan is a
 *   later step's `ride` (whatever that step's plan), never paired -- or, for the backward's last
 *   step under the zero-ahead conditions, arctopk_decode_wire16_scatter.  World size 1 without
 *   communicators packs to bf16 and decodes from it.  ARCTOPK_EINVAL, before anything is enqueued,
 *   for err_in other than 0 / 1, a `sel_stream` other than `stream`, a bound plan as `trail`, and
 *   bucket / err / gerr not 16-B aligned; a `trail` is enqueued on its own, never carried.
 * Replaces: the whole of group_topk_hook's compressed path (:254-290) given the seed.
 */
int arctopk_exchange_step(arctopk_plan* plan, void* bucket, void* err, void* gerr, int32_t ef,
                          int32_t err_in, int32_t draw, uint64_t seed, const arctopk_plan* next,
                          uint64_t next_seed, arctopk_comm* sketch_comm, arctopk_comm* packed_comm,
                          void* stream, void* ar_stream, int32_t defer, arctopk_plan* ride,
                          void* const* ride_marks, arctopk_plan* const* finish,
                          void* const* const* finish_marks, int32_t nfinish, const void* V,
                          void* const* marks, void* sel_stream, arctopk_plan* trail);
/*
 * A TRAILING step (world size 1, EF14 / noef, a deferring caller): the call is recorded on the
 * plan and nothing is enqueued but the projection draw (draw != 0: on `stream`, now).  The next
 * arctopk_exchange_step given it as `trail` carries its encode and select in its own launches
 * (a small bucket then costs no launch of its own); arctopk_exchange_finish enqueues a trailing
 * step that no step carried, then decodes it.  The CONTRACT of a deferred step holds from this
 * call on (bucket, err, gerr untouched until the decode is enqueued).
 */
int arctopk_exchange_trail(arctopk_plan* plan, void* bucket, void* err, void* gerr, int32_t ef,
                           int32_t err_in, int32_t draw, uint64_t seed, const void* V, void* stream);
/* The deferred decode of `plan`'s last deferred exchange step (no-op if none): after that step's
 * packed all-reduce (and, at world size 1, its deferred pack), on the step's select stream if it
 * had one (then `stream` waits for it), else on `stream`.  A trailing step is enqueued first. */
int arctopk_exchange_finish(arctopk_plan* plan, void* stream, void* const* marks);

/*
 * K2 variant for tests/bit-exact checks: the per-row energy keys only
 * (float bits of the energy the reference feeds torch.topk), keys[row_off + row].
 */
int arctopk_row_energy(const arctopk_plan* plan, const void* sketch, int32_t world_size,
                       float* energy, void* stream);

/*
 * K3 pack.  Gather the selected rows into the packed buffer (segment order,
 * ascending rows) and update the local residual.  `rowlist` and `slotmap` are
 * arctopk_select's outputs (rows of 1 or 2 elements are packed by a stream over the
 * slot map, longer rows by gathering the row list):
 *   NONE : packed = G[sel]
 *   EF14 : packed = E[sel] (E holds X after encode); E[sel] = 0
 *   EF21 : D = G[sel] - E[sel]; packed = D; E[sel] = E[sel] + D
 * Replaces: tensor[topk_indices] gathers (:70-71, :101-102), values_memory /
 * indices_memory packing (:116-117), EF14 tensor.view(-1)[indices] = 0 (:124),
 * EF21 zero_/index_put (:126-128) and the residual persistence (:270-275).
 */
int arctopk_pack(const arctopk_plan* plan, const void* grad, void* err, int32_t ef,
                 const int32_t* rowlist, const int32_t* slotmap, void* packed, void* stream);

/*
 * K4 decode.  From the all-reduced packed values:
 *   NONE/EF14 : out = scatter(packed / world_size) into zeros
 *   EF21      : out = gE + scatter(packed / world_size); gE[sel] = out[sel]
 * `out` may alias the bucket (it is the bucket in the hook).  `packed` and `slotmap` are all
 * it reads of the selection: any slot map of arctopk_select's format (per row its slot within
 * the segment, ascending with the row, or -1) and packed values laid out as arctopk_pack
 * writes them, whatever ran on the plan before (the short-row chunks derive their packed
 * ranges from the slot map given, in one extra launch).
 * Replaces: values_memory.div_(ws) (:281), input_tensor.zero_() (:284), the
 * per-tensor index_put scatter (:131-141) and gE.add_/input.copy_ (:288-290).
 */
int arctopk_decode(const arctopk_plan* plan, const void* packed, const int32_t* slotmap,
                   int32_t world_size, int32_t ef, void* gerr, void* out, void* stream);

/*
 * Segment-range forms of K3/K4 (segments [seg_begin, seg_end) only), so a caller can
 * pipeline the packed all-reduce: pack group g, start its collective, pack g+1, ...
 * and decode each group once its collective has completed.  Packed data of the
 * segments in [b, e) occupy packed[seg(b).packed_off, seg(e-1).packed_off + k(e-1)).
 */
int arctopk_pack_segments(const arctopk_plan* plan, int32_t seg_begin, int32_t seg_end,
                          const void* grad, void* err, int32_t ef, const int32_t* rowlist,
                          const int32_t* slotmap, void* packed, void* stream);
int arctopk_decode_segments(const arctopk_plan* plan, int32_t seg_begin, int32_t seg_end,
                            const void* packed, const int32_t* slotmap, int32_t world_size,
                            int32_t ef, void* gerr, void* out, void* stream);

/* ---- TopK / RandK baselines (comm_hooks/sparse_hook.py, sparse_hook_c4.py) ---------- */
/*
 * Bucket-typed buffers (x, vals, E, out, gerr) are of element type `dtype` (ARCTOPK_F32 or
 * ARCTOPK_BF16); bf16 arithmetic rounds after every add / divide, as the reference's torch
 * ops on bf16 tensors do.  Tensors of a bucket are described by host arrays of `ntensors` entries:
 * offsets[i] (element offset in the bucket), numels[i], ks[i] (= max(1, int(numel*ratio)),
 * sparse_hook.py:77-78) and k_off[i] (offset of tensor i's k entries in the packed
 * idx/vals buffers).  Up to ARCTOPK_SPARSE_MAX_BATCH tensors go into one launch; more
 * are processed in batches.
 */
#define ARCTOPK_SPARSE_MAX_BATCH 64

/*
 * Bytes of `workspace` that arctopk_topk_select needs for these tensor sizes (fixed
 * tables plus a candidate list of ~n/8 per tensor of a launch batch), or
 * -ARCTOPK_EINVAL for bad arguments.
 */
int64_t arctopk_sparse_workspace_bytes(int32_t ntensors, const int64_t* numels);

/*
 * Exact element top-k of |x| per tensor by multi-block radix select; ties at the
 * k-th |x|: lowest index first.  Writes each tensor's k indices ascending as int32
 * (idx[k_off[i] ..]) and the values x[idx] (vals[k_off[i] ..]).
 * Replaces: torch.topk(tensor.abs(), k, sorted=False), .to(int32), tensor[indices]
 * (sparse_hook.py:26-28, :97-98).  zero_selected = 1: x (non-const here) is also written
 * back with its selected elements zeroed, in the same pass (EF14's `tensor[indices] = 0`,
 * :104, when x is the residual E after arctopk_ef14_fold).
 */
int arctopk_topk_select(const void* x, int32_t ntensors, const int64_t* offsets,
                        const int64_t* numels, const int64_t* ks, const int64_t* k_off,
                        int32_t* idx, void* vals, void* workspace, int32_t dtype,
                        int32_t zero_selected, void* stream);

/*
 * RandK, device-side index source (the performance mode; the parity mode draws torch.randperm
 * on the host, sparse_hook.py:20): tensor i's k indices are those of its k largest keys
 * key(j) = rk(s_i, j), a keyed bijection of the index j (two xorshift-multiply rounds; s_i =
 * splitmix64(seed + 0x9E3779B97F4A7C15 * (i + 1)) truncated to 32 bits), so the keys are
 * distinct and the subset is a uniformly random k-subset of [0, numel_i).  They are selected by
 * the same exact multi-block radix select as arctopk_topk_select and written ASCENDING
 * (idx[k_off[i] ..]), so every later pass streams the tensor in order.  x != NULL: also
 * vals = x[offsets[i] + idx] and (zero_selected) x written back with those entries zeroed in
 * the same pass (EF14's residual, sparse_hook.py:104, x = E after arctopk_ef14_fold); x = NULL:
 * indices only (offsets / vals NULL, zero_selected 0).  workspace: arctopk_sparse_workspace_bytes.
 * Replaces: torch.randperm(numel, device=...)[:k] + tensor[indices] (sparse_hook.py:20-22).
 */
int arctopk_randk_select(const void* x, int32_t ntensors, const int64_t* offsets,
                         const int64_t* numels, const int64_t* ks, const int64_t* k_off,
                         uint64_t seed, int32_t* idx, void* vals, void* workspace, int32_t dtype,
                         int32_t zero_selected, void* stream);
/*
 * arctopk_topk_select on x = E with EF14 applied in the select's first pass (fp32 only, every
 * tensor 16-B aligned with numel % 4 == 0; ARCTOPK_EINVAL otherwise, and nothing is enqueued):
 * that pass streams g (the bucket) and E, writes E := g + E (err_in; else E := g, the first call)
 * -- tensor.add_(E) (sparse_hook.py:205) -- and histograms it; the later passes select, gather and
 * (:104) zero E as arctopk_topk_select(E, ..., zero_selected = 1) does.  g is not written.
 * Replaces arctopk_ef14_fold followed by that select: one pass over the bucket and the residual
 * fewer.
 */
int arctopk_topk_select_ef14(const void* g, void* E, int32_t err_in, int32_t ntensors,
                             const int64_t* offsets, const int64_t* numels, const int64_t* ks,
                             const int64_t* k_off, int32_t* idx, void* vals, void* workspace,
                             int32_t dtype, void* stream);
/*
 * The same RandK draw with EF14 applied in the select's write pass (the hash keys never read the
 * data, so the passes before it do not either): v = g + E (err_in; else v = g, the first call),
 * rounded to the dtype as tensor.add_(E) is (sparse_hook.py:205), vals = v[idx], and E := v with
 * the selected elements zeroed (:104).  g (the bucket) is not written.  Replaces arctopk_ef14_fold
 * followed by arctopk_randk_select(E, ..., zero_selected = 1): one pass over the bucket and the
 * residual instead of two.
 */
int arctopk_randk_select_ef14(const void* g, void* E, int32_t err_in, int32_t ntensors,
                              const int64_t* offsets, const int64_t* numels, const int64_t* ks,
                              const int64_t* k_off, uint64_t seed, int32_t* idx, void* vals,
                              void* workspace, int32_t dtype, void* stream);

/*
 * Row- and column-wise selection (sparse_type "row" / "column": sparsify_by_row, sparsify_by_column,
 * sparse_hook.py:36-75).  Tensor i is viewed as [rows[i], cols[i]] (row-major at offsets[i]);
 * by_column = 0: every row is a segment of cols[i] contiguous elements; by_column = 1: every column
 * is a segment of rows[i] elements at stride cols[i].  Each segment takes its own k_seg[i] keys
 * (1 <= k_seg <= segment length), so tensor i has nseg * k_seg[i] entries from k_off[i] on.
 *   hashed = 0 (TopK): the k_seg largest |x| of the segment, ties at the threshold lowest position
 *     in the segment first.
 *   hashed = 1 (RandK): the k_seg largest keys rk(hseed(i, s), j) over the positions j of segment s
 *     (rk: arctopk_randk_select's keyed bijection), with
 *     hseed(i, s) = low32(fin(seed + 0x9E3779B97F4A7C15 * (i + 1) + 0xD1B54A32D192ED03 * s)) mod 2^64,
 *     fin the splitmix64 finaliser; hseed(i, 0) is arctopk_randk_select's seed of tensor i, so a
 *     one-segment tensor draws what that entry draws.
 * idx holds int32 flat indices into the tensor (row * cols + column):
 *   by_column = 0: segment-major, ascending within a segment -- ascending over the tensor;
 *   by_column = 1: the reference's [k_seg, cols] layout: entry j of column c is at
 *     k_off[i] + j * cols + c and holds row_j(c) * cols + c with row_0(c) < row_1(c) < ...
 * x != NULL: vals = x[offsets[i] + idx] in the same layout, and with zero_selected x is written
 * back with those elements zeroed in the same pass (EF14 on E); x = NULL needs hashed: indices
 * only (offsets / vals NULL, zero_selected 0).  ARCTOPK_EINVAL, with nothing enqueued, for null
 * arrays, rows * cols outside [1, 2^31), k_seg outside [1, segment length] or a bad dtype.
 * Row segments longer than 12,288 keys go through the multi-block select of arctopk_topk_select
 * (one item per segment); column strips re-read their keys from memory and have no row limit.
 * workspace: arctopk_seg_workspace_bytes of the same geometry (-ARCTOPK_EINVAL for a bad one).
 */
int64_t arctopk_seg_workspace_bytes(int32_t ntensors, const int64_t* rows, const int64_t* cols,
                                    const int64_t* k_seg, int32_t by_column);
int arctopk_seg_select(void* x, int32_t ntensors, const int64_t* offsets, const int64_t* rows,
                       const int64_t* cols, const int64_t* k_seg, const int64_t* k_off,
                       int32_t by_column, int32_t hashed, uint64_t seed, int32_t* idx, void* vals,
                       void* workspace, int32_t dtype, int32_t zero_selected, void* stream);

/* Gather vals[k_off[i] + j] = x[offsets[i] + idx[k_off[i] + j]]  (sparse_hook.py:22). */
int arctopk_sparse_gather(const void* x, int32_t ntensors, const int64_t* offsets,
                          const int64_t* ks, const int64_t* k_off, const int32_t* idx,
                          void* vals, int32_t dtype, void* stream);

/*
 * Residual persistence at the selected entries (sparse_hook.py:103-109, :257-267):
 *   EF14 : E[off + idx] = 0        (E already holds x = G + E_prev, see arctopk_ef_apply)
 *   EF21 : E[off + idx] = E + decay * vals, one rounding (E.add_(C(G - E), alpha=error_decay),
 *          :265; C(.) is zero elsewhere; decay = 1 is the default state)
 */
int arctopk_sparse_residual(void* E, int32_t ntensors, const int64_t* offsets,
                            const int64_t* ks, const int64_t* k_off, const int32_t* idx,
                            const void* vals, int32_t ef, float decay, int32_t dtype, void* stream);

/*
 * Decode into `out` (every element written):
 *   accumulate = 0 (RandK): out = 0; out[off + idx[j]] = vals[j] / world_size     (:273-278)
 *   accumulate = 2 (RandK, each tensor's idx ascending: arctopk_randk_select): the same, as one
 *                           pass of whole chunks (zeros and values composed in LDS)
 *   accumulate = 1 (TopK) : out = 0; for rank q = 0..nranks-1 in order:
 *                           out[off + idx_q[j]] += vals_q[j]; then out /= world_size (:285-292)
 *   accumulate = 3 (TopK, idx in any order: arctopk_seg_select's column layout): the same sums
 *                           in the same rank order, as a memset and one scatter per rank
 * `vals`/`idx` hold nranks consecutive payloads of packed_len entries each.
 * EF21 (gerr != NULL): gE = gE + decay * out (one rounding: gE.add_(out, alpha=error_decay));
 * out = gE (:295-297).
 */
int arctopk_sparse_decode(void* out, int64_t numel, int32_t ntensors, const int64_t* offsets,
                          const int64_t* ks, const int64_t* k_off, int64_t packed_len,
                          const int32_t* idx, const void* vals, int32_t nranks,
                          int32_t world_size, int32_t accumulate, void* gerr, float decay,
                          int32_t dtype, void* stream);

/*
 * EF pre-apply on a whole bucket, one pass (ARC-TopK fuses this into arctopk_encode):
 *   EF14 : x = x + E (err_in = 1) or x unchanged (first call); then E = x
 *   EF21 : x = x - E
 * Replaces: input_tensor.add_(error_dict[b], alpha=+-1) (sparse_hook.py:205, :212) and the
 * full-bucket E.copy_(input_tensor) of EF14 (:258).
 */
int arctopk_ef_apply(void* x, void* E, int64_t numel, int32_t ef, int32_t err_in, int32_t dtype,
                     void* stream);

/*
 * EF14 fold for the sparse hooks: E := x + E (err_in = 1) or E := x (first call); x is not
 * written.  The caller then selects / gathers from E (which holds the pre-compression
 * bucket) and decodes into x.  Replaces input_tensor.add_(E) (sparse_hook.py:205) and the
 * full-bucket E.copy_(input_tensor) (:258).  With arctopk_topk_select(..., zero_selected=1)
 * on E, the EF14 residual `E[indices] = 0` (:104) is done in the select's last pass.
 */
int arctopk_ef14_fold(const void* x, void* E, int64_t numel, int32_t err_in, int32_t dtype,
                      void* stream);

/* ---- TopK / RandK baselines: fp32 residuals under a bf16 bucket (SparseState.error_dtype) ---- */
/*
 * In this section bucket-typed buffers (g, vals, out) are bf16 and residual buffers (E, D, gE,
 * scratch) are fp32, whatever the names' meaning elsewhere.  f = bf16 -> fp32 (exact), b = fp32 ->
 * bf16 (round to nearest even, NaN -> 0x7FC0).  Indices come from the existing selects run on the
 * fp32 buffer with dtype = ARCTOPK_F32 and zero_selected = 0 (arctopk_topk_select,
 * arctopk_seg_select, arctopk_randk_select); the values leave as bf16, so the exchange and EF14's
 * decode (arctopk_sparse_decode, dtype = ARCTOPK_BF16) are the bf16 path's.  Tensor i's extent is
 * offsets[i + 1] - offsets[i] (the last one's ends at numel): the tensors tile the bucket in order.
 */

/*
 * EF pre-apply of a whole bucket into the fp32 buffers, one pass; g is not written:
 *   EF14 : E := f(g) + E (err_in = 1; one fp32 add) or E := f(g) (first call; E is not read); D unused
 *   EF21 : D := f(g) - E (one fp32 subtract); E is not written
 * g, E and D 16-B aligned: 16 B of g and 2 x 16 B of fp32 in and out per unit of 8 elements,
 * nontemporal, several units' loads in flight before the first store, and the last numel % 8
 * elements one by one; otherwise element by element.  ARCTOPK_EINVAL for a null g or E (EF21: D), an
 * ef other than EF14 / EF21 or a pointer not aligned to its element.
 * Replaces: input_tensor.add_(E, alpha=+-1) (sparse_hook.py:205, :212) and EF14's full-bucket
 * E.copy_(input_tensor) (:258), as arctopk_ef14_fold / arctopk_ef_apply do for one dtype.
 */
int arctopk_sparse_fold_mixed(const void* g, void* E, void* D, int64_t numel, int32_t ef,
                              int32_t err_in, void* stream);

/*
 * Gather and residual at the selected elements: for tensor i and j < ks[i], with
 * e = offsets[i] + idx[k_off[i] + j],
 *   vals[k_off[i] + j] = b(src[e])
 *   EF14 (src == E, after the fold): E[e] := src[e] - f(vals)   (exact: what the bf16 wire drops)
 *   EF21 (src == D)                : E[e] := fma(decay, f(vals), E[e])   (one rounding)
 * Other elements of E are untouched.  Every index is checked against its tensor's extent: one
 * outside it writes vals = 0 and nothing else.  One launch per ARCTOPK_SPARSE_MAX_BATCH tensors;
 * ARCTOPK_EINVAL, with nothing enqueued, for null arrays, tensors that do not tile [offsets[0],
 * numel) in order, a k outside [1, extent], EF14 with src != E, or an ef other than EF14 / EF21.
 * Replaces: tensor[indices] (sparse_hook.py:22, :28), `tensor[indices] = 0` (:104) and
 * E.add_(C(G - E), alpha=error_decay) (:265) -- arctopk_sparse_gather + arctopk_sparse_residual.
 */
int arctopk_sparse_pack_mixed(const void* src, void* E, int64_t numel, int32_t ntensors,
                              const int64_t* offsets, const int64_t* ks, const int64_t* k_off,
                              const int32_t* idx, void* vals, int32_t ef, float decay, void* stream);

/*
 * EF21 decode: scratch (numel fp32) := 0, then for rank q = 0..nranks-1 in order
 * scratch[off + idx_q[j]] += f(vals_q[j]) (indices within a payload are distinct; checked against
 * the tensor's extent, one outside it is skipped); then on every element
 *   m = scratch / world_size (correctly rounded: x 1/ws for a power of two, else a division)
 *   gE := fma(decay, m, gE);  out = b(gE)
 * (m = 0 where nothing was selected: gE keeps its bits except a stored -0.0, as gE + 0.0 does).
 * RandK passes its all-reduced payload with nranks = 1.  `vals` / `idx` hold nranks consecutive
 * payloads of packed_len entries.  out, gE and scratch 16-B aligned: units of 8 elements as the
 * fold's; otherwise element by element.
 * Replaces: the scatter(-add) / ws of sparse_hook.py:273-292 and gE.add_(out, alpha=error_decay);
 * out = gE (:295-297) -- arctopk_sparse_decode with gerr, without its roundings to bf16.
 */
int arctopk_sparse_decode_mixed21(void* out, void* gE, void* scratch, int64_t numel,
                                  int32_t ntensors, const int64_t* offsets, const int64_t* ks,
                                  const int64_t* k_off, int64_t packed_len, const int32_t* idx,
                                  const void* vals, int32_t nranks, int32_t world_size, float decay,
                                  void* stream);

/* ---- TopK / RandK baselines: bf16 values on the wire of an fp32 bucket (SparseState.wire_dtype) ---- */
/*
 * In this section the bucket (out), the selects' values and the residuals (E, gE) are fp32 and the
 * payload's values (vals16) are bf16; f and b as above.  Fold and selection are the fp32 path's,
 * unchanged; these two entries replace arctopk_sparse_residual and arctopk_sparse_decode behind
 * them.  Tensor i's extent is offsets[i + 1] - offsets[i] (the last one's ends at numel): the
 * tensors tile [offsets[0], numel) in order.  Both entries check every argument and every batch
 * of the layout before any device call (host-testable) and return ARCTOPK_EINVAL, with nothing
 * enqueued, for a null array, ntensors < 1, numel < 1, tensors that do not tile in order, a k
 * outside [1, extent], or a pointer not aligned to its element.
 */

/*
 * Round the selected values to the wire and keep what the rounding drops: for tensor i and
 * j < ks[i], with p = k_off[i] + j and e = offsets[i] + idx[p],
 *   vals16[p] = b(values[p])
 *   EF_NONE : nothing else (E may be NULL)
 *   EF14    : E[e] := values[p] - f(vals16[p])   (one exact fp32 subtract; a store, so it holds
 *             whether or not the select has zeroed E[e] already)
 *   EF21    : E[e] := fma(decay, f(vals16[p]), E[e])   (one rounding)
 * `values` are the selects' contiguous fp32 values (arctopk_topk_select, arctopk_randk_select,
 * arctopk_seg_select, their _ef14 forms, or arctopk_sparse_gather).  Other elements of E are
 * untouched; an index outside its tensor's extent writes vals16 = 0 and nothing else.  One launch
 * per ARCTOPK_SPARSE_MAX_BATCH tensors; a tensor whose slice of the payload is 16-B aligned goes
 * in units of 4 (16 B of indices and values in, 8 B out), the rest element by element.
 * ARCTOPK_EINVAL also for an unknown ef, or EF14 / EF21 with a null E.
 */
int arctopk_sparse_pack_wire16(const void* values, void* E, int64_t numel, int32_t ntensors,
                               const int64_t* offsets, const int64_t* ks, const int64_t* k_off,
                               const int32_t* idx, void* vals16, int32_t ef, float decay, void* stream);

/*
 * Decode bf16 payloads into the fp32 bucket (every element written).  `accumulate` has the values
 * of arctopk_sparse_decode: 0 RandK, any order; 1 TopK, each tensor's idx ascending on every rank;
 * 2 RandK ascending; 3 TopK, any order.  Per element
 *   s = 0.0f + f(v_0) + f(v_1) + ...   the ranks' values at that element, added in rank order in
 *                                      fp32 (TopK: nranks payloads; RandK: the one all-reduced)
 *   m = s / world_size                 correctly rounded (x 1/ws for a power of two, else a division)
 *   gE == NULL : out = m  (0 where no rank selected the element)
 *   gE != NULL : gE := fma(decay, m, gE);  out = gE   (EF21; on every element)
 * Indices within a payload are distinct; one outside its tensor's extent is skipped.  `vals16` /
 * `idx` hold nranks consecutive payloads of packed_len entries.
 * accumulate 1 or 2 with offsets[0] == 0 takes the merged route: one launch per
 * ARCTOPK_SPARSE_MAX_BATCH tensors in which a block composes a 4096-element chunk of a tensor from
 * all ranks' slices in LDS, in rank order, and writes it once with mean and gE applied -- no
 * memset, no read-modify-write of the bucket, no separate divide pass.  Anything else takes the
 * scattered route: memset, one scatter launch per rank, one finalize pass.  Both give the same bits.
 * ARCTOPK_EINVAL also for nranks < 1, world_size < 1, packed_len < k_off[i] + ks[i], or accumulate
 * outside 0..3.
 */
int arctopk_sparse_decode_wire16(void* out, int64_t numel, int32_t ntensors, const int64_t* offsets,
                                 const int64_t* ks, const int64_t* k_off, int64_t packed_len,
                                 const int32_t* idx, const void* vals16, int32_t nranks,
                                 int32_t world_size, int32_t accumulate, void* gE, float decay,
                                 void* stream);

/*
 * Momentum fold of a whole bucket, in place, stream-ordered, one launch per
 * ARCTOPK_SPARSE_MAX_BATCH tensors: for every tensor i,
 *   bucket[offsets[i] + j] = one_minus_beta * bucket[offsets[i] + j] + beta * moments[i][j],
 * j < numels[i], rounded as the two torch ops round on the GPU: the product to the bucket's
 * type, then one fused multiply-add of the moment rounded to it again; the scalars are the
 * Python doubles (1 - beta1, beta1), cast to fp32 as torch casts them.
 * offsets / numels / moments are host arrays of ntensors entries (element offsets into the
 * bucket; moments[i] a device pointer to numels[i] contiguous elements of mom_dtype, any
 * element-aligned address).  (dtype, mom_dtype) is (F32, F32), (BF16, BF16) or (BF16, F32);
 * ARCTOPK_EDTYPE otherwise.  ARCTOPK_EINVAL for a null array or bucket, ntensors < 0, a
 * negative offset or numel, a null moment with numel > 0, or a bucket / moment pointer not
 * aligned to its element size; every check runs before any device call (host-testable).
 * Tensors with numel 0 are skipped; ntensors == 0 enqueues nothing.  No allocation, no
 * host-to-device copy, no synchronisation.
 * Replaces: the per-parameter loop grad.mul_(1 - self.beta1).add_(exp_avg, alpha=self.beta1)
 * of HookState.accumulate_momentum_on_bucket (comm_hooks/utils.py:54-65).
 */
int arctopk_momentum_fold(void* bucket, int32_t ntensors, const int64_t* offsets,
                          const int64_t* numels, const void* const* moments,
                          double one_minus_beta, double beta,
                          int32_t dtype, int32_t mom_dtype, void* stream);

/*
 * EF14 with an fp32 residual under a bf16 bucket: the encode and pack
 * phases of a bf16 plan whose residual `err_f32` holds plan.numel floats.  f = bf16 -> fp32
 * (exact), b = fp32 -> bf16 as every bf16 value of the library is rounded (arctopk_round_bf16).
 *   arctopk_encode_mixed : X = f(G) + E (err_in = 1) or f(G) (err_in = 0), one fp32 add; E := X;
 *       sketch[SKETCH seg] = b(X.view(n, m) @ f(V)) (fp32 sums, one rounding), sketch[RAW seg] =
 *       b(X); a DENSE segment has no encode work.  V and the sketch are the plan's bf16 layouts.
 *   arctopk_pack_mixed   : every selected row (rowlist: arctopk_select's): packed = b(X), X read
 *       from E; E := X - f(packed), one fp32 subtract (EF14's E = X - C[X]: the residual keeps the
 *       rounding remainder of what was sent); other rows keep E = X.  A DENSE segment forms
 *       X = f(G) + E (err_in, as given to the encode) here, every element selected; `grad` may be
 *       NULL for a plan without DENSE segments.  The slot map is not written.
 * Select and decode are arctopk_select and arctopk_decode(ef = ARCTOPK_EF14) on the same buffers.
 * At world size 1 the decoded bucket satisfies f(out) + E_new == f(G) + E_old on every element.
 * ARCTOPK_EINVAL for a plan that is not ARCTOPK_BF16, err_in outside {0, 1}, a null pointer the
 * plan needs, or grad / err / packed not 16-B aligned.  Stream-ordered, no host synchronisation;
 * the first of these calls on a plan builds its work tables (one allocation and copy, freed with
 * the plan), every later one only enqueues.  err_in = 2 (zero rows) does not exist here: the
 * selected rows of E are not zero.
 * Replaces: input_tensor.add_(error) (:227), tensor @ V (:53, :83), the gathers (:70-71,
 * :101-102) and EF14's tensor.view(-1)[indices] = 0 (:124) for a residual kept in fp32.
 */
int arctopk_encode_mixed(const arctopk_plan* plan, const void* grad_bf16, float* err_f32,
                         int32_t err_in, const void* V_bf16, void* sketch_bf16, void* stream);
int arctopk_pack_mixed(const arctopk_plan* plan, const void* grad_bf16, float* err_f32,
                       int32_t err_in, const int32_t* rowlist, const int32_t* slotmap,
                       void* packed_bf16, void* stream);

/*
 * EF21 with both residuals in fp32 under a bf16 bucket: the encode, pack
 * and decode phases of a bf16 plan whose local residual `err_f32` (E) and global residual
 * `gerr_f32` (gE) hold plan.numel floats each.  f and b as above.
 *   arctopk_encode_mixed21 : D = f(G) - E, one fp32 subtract; sketch[SKETCH seg] =
 *       b(D.view(n, m) @ f(V)) (fp32 sums, one rounding), sketch[RAW seg] = b(D); a DENSE segment
 *       has no encode work.  Nothing but the sketch is written: E is read only.
 *   arctopk_pack_mixed21   : every selected row (rowlist: arctopk_select's; every entry is checked
 *       against the segment's rows) and every element of a DENSE segment: D as above, packed =
 *       b(D), E := E + f(packed), one fp32 add (EF21's E += C[G - E] with C what was sent: the
 *       rounding remainder D - f(packed) stays in G - E).  Other rows are not touched.  The slot
 *       map is not written.
 *   arctopk_decode_mixed21 : `packed` holds the all-reduced values.  A selected element (slot map:
 *       arctopk_select's; every element of a DENSE segment): gE := gE + f(P) / world_size, the
 *       correctly rounded fp32 quotient, not rounded to bf16 before the add.  out = b(gE) on every
 *       element of the bucket; gE of unselected rows is read and left as stored.  `out` may be the
 *       bucket itself.
 * Select is arctopk_select on the same buffers.  At world size 1, gE == E bit for bit after every
 * call of a bucket whose first call set E = f(G), gE = f(out).
 * ARCTOPK_EINVAL for a plan that is not ARCTOPK_BF16, a null pointer, world_size < 1, or grad /
 * err / gerr / packed / out not 16-B aligned.  Stream-ordered, no host synchronisation; work tables
 * as for arctopk_encode_mixed (the same ones, with the decode's tiles).
 * Replaces: input_tensor.add_(error, alpha=-1.0) (:234), tensor @ V (:53, :83), the gathers
 * (:70-71, :101-102), EF21's error.add_(input_tensor) (:275) and global_error.add_(input_tensor);
 * input_tensor.copy_(global_error) (:289-290) for residuals kept in fp32.
 */
int arctopk_encode_mixed21(const arctopk_plan* plan, const void* grad_bf16, const float* err_f32,
                           const void* V_bf16, void* sketch_bf16, void* stream);
int arctopk_pack_mixed21(const arctopk_plan* plan, const void* grad_bf16, float* err_f32,
                         const int32_t* rowlist, const int32_t* slotmap, void* packed_bf16,
                         void* stream);
int arctopk_decode_mixed21(const arctopk_plan* plan, const void* packed_bf16, const int32_t* slotmap,
                           int32_t world_size, float* gerr_f32, void* out_bf16, void* stream);

/*
 * The packed values of an fp32 bucket sent as bf16: the pack and decode
 * phases of an fp32 plan whose packed all-reduce carries `packed_bf16`, bf16 values in the plan's
 * packed layout counted in elements (the same packed_off and packed_len: a segment's values start
 * 8-B aligned, 16-B aligned only where packed_off % 8 == 0).  Bucket, residuals, sketch and
 * projections are fp32; encode and select are arctopk_encode and arctopk_select.  f and b as above.
 *   arctopk_pack_wire16   : every selected row (rowlist: arctopk_select's; every entry is checked
 *       against the segment's rows), every selected element of a RAW segment and every element of a
 *       DENSE segment:
 *         NONE : packed = b(G)
 *         EF14 : X read from E (the encode stored it; a DENSE segment forms X = G + E, err_in = 1,
 *                or X = G, err_in = 0, here: one fp32 add); packed = b(X); E := X - f(packed), one
 *                fp32 subtract (exact: the residual keeps the rounding remainder of what was sent);
 *                other rows keep E = X
 *         EF21 : D = G - E, one fp32 subtract; packed = b(D); E := E + f(packed), one fp32 add;
 *                other rows are not touched
 *       Neither the row list nor the slot map is written, and the plan's zero-rows record is not
 *       set: err_in = 2 does not exist here, a selected row of E holds its remainder, not zero.
 *   arctopk_decode_wire16 : `packed_bf16` holds the all-reduced values P; mean = f(P) / world_size,
 *       the correctly rounded fp32 quotient, not rounded to bf16.
 *         NONE, EF14 : out = mean on selected elements (slot map: arctopk_select's; every element of
 *                a DENSE segment), 0 elsewhere
 *         EF21 : gE := gE + mean on selected elements, one fp32 add; out = gE on every element; gE
 *                of unselected rows is read and left as stored
 *       Every element of `out` is written; `out` may be the bucket.
 * At world size 1: EF14 leaves out + E_new == G + E_old on every element, bit for bit; EF21 leaves
 * gE == E bit for bit after every call of a bucket whose first call set E = G, gE = out.
 * ARCTOPK_EINVAL for a null plan or one that is not ARCTOPK_F32, ef outside NONE / EF14 / EF21,
 * err_in outside {0, 1}, world_size < 1, a null pointer the mode needs (rowlist, slotmap, packed,
 * out; err for EF14 and EF21; gerr for EF21; grad for NONE, for EF21, and for EF14 on a plan with
 * DENSE segments), grad / err / gerr / out not 16-B aligned, or packed_bf16 not 8-B aligned; every
 * check runs before any device call and nothing is enqueued when one fails.  Stream-ordered, no
 * host synchronisation; the first of these calls on a plan builds its work tables (one allocation
 * and copy, freed with the plan), every later one only enqueues.
 * Replaces: the gathers (:70-71, :101-102), EF14's tensor.view(-1)[indices] = 0 (:124), EF21's
 * zero_/index_put (:126-128) and error.add_(input_tensor) (:275), values_memory.div_(ws) (:281),
 * input_tensor.zero_() (:284), the scatter (:131-141) and gE.add_/input.copy_ (:288-290), for
 * values_memory (:261-263) carried as bf16 on the wire.
 */
int arctopk_pack_wire16(const arctopk_plan* plan, const void* grad, void* err, int32_t ef, int32_t err_in,
                        const int32_t* rowlist, const int32_t* slotmap, void* packed_bf16, void* stream);
int arctopk_decode_wire16(const arctopk_plan* plan, const void* packed_bf16, const int32_t* slotmap,
                          int32_t world_size, int32_t ef, void* gerr, void* out, void* stream);
/*
 * The bf16-wire decode of NONE / EF14 into an `out` that is already zero (the zero-ahead drain of
 * the exchange step's last bucket): for every selected row (rowlist: arctopk_select's; every entry is
 * checked against the segment's rows), every selected element of a RAW segment and every element of
 * a DENSE segment, out = f(P) / world_size, the mean arctopk_decode_wire16 forms; nothing else is
 * read or written (2 B read and 4 B written per selected element, against 4 B per bucket element
 * plus 2 B per selected one for the whole decode).  The result equals arctopk_decode_wire16's with
 * ef NONE or EF14 when `out` was zero.  ARCTOPK_EINVAL for a null plan or one that is not
 * ARCTOPK_F32, a null packed_bf16 / rowlist / slotmap / out, world_size < 1, `out` not 16-B aligned
 * or packed_bf16 not 8-B aligned; nothing is enqueued then.  `slotmap` is not read.
 */
int arctopk_decode_wire16_scatter(const arctopk_plan* plan, const void* packed_bf16, const int32_t* rowlist,
                                  const int32_t* slotmap, int32_t world_size, void* out, void* stream);
/*
 * Binds `packed_bf16` (8-B aligned, packed_len bf16 elements, the plan's packed layout; NULL
 * unbinds) to an ARCTOPK_F32 plan: its exchange steps (arctopk_exchange_step) then run on the bf16
 * wire -- the pack is arctopk_pack_wire16's, the packed all-reduce moves `packed_bf16` as
 * ARCTOPK_BF16 and the decode is arctopk_decode_wire16's (arctopk_decode_wire16_scatter for the
 * zero-ahead drain) -- with the deferral, all-reduce stream and watchdog of any other step.  Such a
 * step takes no select stream, no trailing step's launches, no err_in = 2, and its decode rides in
 * no other launch.  ARCTOPK_EINVAL for a plan that is not ARCTOPK_F32, a misaligned buffer, or a
 * plan with a step deferred or trailing.  A plan without the binding runs the default step.
 */
int arctopk_plan_bind_wire16(arctopk_plan* plan, void* packed_bf16);

/*
 * Device projections of one bucket call: for every SKETCH segment in bucket order,
 * V[v_off ..] = torch.randn(m, r, device=dev, dtype) as drawn by the reference on the GPU
 * right after torch.manual_seed(seed) (group_topk_hook_no_reshape.py:49, :79, :255):
 * torch's Philox4x32-10 normal_ kernel (hiprand) reproduced element by element, bit for bit.
 * Stream-ordered, one launch.  arctopk_plan_philox_advance: the device generator's Philox
 * offset after those draws (what torch.manual_seed + the reference's draws leave behind).
 * On a plan with ARCTOPK_PLAN_RESTART_DRAWS every tensor's V starts at Philox offset 0 of `seed`
 * (torch.empty(m, r, device=dev).normal_(generator=g), g a fresh device generator seeded with
 * `seed`, c4 :31-39) and the advance is 0: the global generator is not drawn from.
 */
int arctopk_draw_projections(const arctopk_plan* plan, uint64_t seed, void* V, void* stream);
int arctopk_plan_philox_advance(const arctopk_plan* plan, uint64_t* advance);

/*
 * Host-only (no GPU): `total` (a multiple of 16) consecutive values of the reference's
 * bf16 projection stream -- torch.randn(..., dtype=bfloat16) on CPU after
 * torch.manual_seed(seed) (group_topk_hook_no_reshape.py:49, :79, :255) -- as bf16 bit
 * patterns.  Valid when every tensor's m*r is a multiple of 16 (no tail recompute).
 * Replaces torch's scalar BFloat16 normal_fill (~8x slower) in the projection prefetch.
 */
int arctopk_draw_bf16_normal(uint64_t seed, int64_t total, uint16_t* out);

/*
 * Host-only (no GPU): one bucket call's projections -- for each of `ntensors` tensors in
 * bucket order, sizes[t] = m_t * r values of torch.randn(m_t, r, dtype) on CPU, all drawn
 * from ONE generator stream after torch.manual_seed(seed) (group_topk_hook_no_reshape.py:49,
 * :79, :255) -- concatenated into `out` (dtype ARCTOPK_F32: float, ARCTOPK_BF16: bf16 bit
 * patterns).  Replaces the reference's per-tensor torch.randn calls (one torch dispatch and
 * Python round trip each) with one call that runs without the GIL.
 */
int arctopk_draw_normal(uint64_t seed, int32_t dtype, int32_t ntensors, const int64_t* sizes,
                        void* out);

/*
 * Host-only: a pool of native threads drawing projections ahead (arctopk_draw_normal into
 * caller-owned buffers that must stay alive until the draw is waited or polled complete).
 * submit returns a ticket (> 0) or -status; wait blocks until that draw is done and returns
 * its status; poll returns 1 when done, -status if the draw failed (ticket then forgotten
 * either way), 0 if still pending.
 * destroy drops queued draws and joins the threads (running draws finish).
 */
int arctopk_draw_pool_create(int32_t nthreads, void** pool);
int arctopk_draw_pool_destroy(void* pool);
int64_t arctopk_draw_submit(void* pool, uint64_t seed, int32_t dtype, int32_t ntensors,
                            const int64_t* sizes, void* out);
int arctopk_draw_wait(void* pool, int64_t ticket);
int arctopk_draw_poll(void* pool, int64_t ticket);

/* Stream-ordered host -> device copy (hipMemcpyAsync), for the projection ring. */
int arctopk_memcpy_h2d_async(void* dst, const void* src, int64_t bytes, void* stream);

/*
 * Device-scope stream events for the hook's own intra-device ordering (projection copy ->
 * encode, encode -> reuse of a projection slot).  torch's events release to system scope:
 * recording one between two kernels writes back the L2 and leaves the GPU idle for several
 * microseconds; these use hipEventReleaseToDevice | hipEventDisableTiming.  No reference
 * counterpart (the reference is synchronous).
 *   query: 0 = complete, 1 = not yet, < 0 / other = HIP error.
 */
int arctopk_event_create(void** event);
int arctopk_event_destroy(void* event);
int arctopk_event_record(void* event, void* stream);
int arctopk_event_wait(void* stream, void* event);
int arctopk_event_query(void* event);
/* Timing variant (hipEventReleaseToDevice, timing enabled) for per-kernel durations in
 * bench.py: a torch event between two kernels writes back the L2 to system scope, which
 * adds several microseconds to the interval it brackets; these measure what the kernel
 * trace measures.  elapsed: milliseconds between two completed records. */
int arctopk_event_create_timed(void** event);
int arctopk_event_elapsed_ms(float* ms, void* start, void* end);

/* Test entry point: the kernels' fp32 -> bf16 rounding (RNE, NaN -> 0x7FC0) of n device
 * values, to check it against c10::BFloat16 on the host. */
int arctopk_round_bf16(const float* in, uint16_t* out, int64_t n, void* stream);

/* Diagnostics (not part of the codec): with ARCTOPK_HOST_TIMING=1 in the environment at the
 * first exchange step, the host nanoseconds each part of arctopk_exchange_step took, summed over
 * the steps since the last read -- ns[0 .. min(n, 8)) = entry, encode, sketch all-reduce, select,
 * pack, packed all-reduce, finish, decode; *calls = steps summed -- and the sums are reset.
 * All zero when the variable is unset.  (bench.py --host-timing breakdowns) */
int arctopk_diag_host_times(int64_t* ns, int32_t n, int64_t* calls);
/* Encode launches of `plan` so far that ran the zero-rows kernel (err_in = 2 accepted; see
 * arctopk_encode).  Tests use it to show the path was taken or refused. */
int arctopk_diag_zero_row_encodes(const arctopk_plan* plan, int64_t* count);
/* Exchange steps of `plan` so far whose decode was the bf16-wire zero-ahead scatter
 * (arctopk_plan_bind_wire16, arctopk_decode_wire16_scatter). */
int arctopk_diag_wire16_scatters(const arctopk_plan* plan, int64_t* count);
/* Which encode paths `plan` holds, from its host-side bookkeeping (nothing is launched):
 * out[0 .. min(n, ARCTOPK_DIAG_ENCODE_TILES)) =
 *   [0] .. [3]  encode tiles of the plan's default table per mode: 1-D pass-through (RAW),
 *               thread-per-row LDS tile, wave-per-row with 16-byte loads, wave-per-row scalar;
 *   [4]         column-split tensors;
 *   [5]         tensors whose encode writes select keys (world size 1);
 *   [6]         1 when the table runs the short-row encode kernel, else 0;
 *   [7], [8]    a bf16 plan's fp32-residual encode (arctopk_encode_mixed / _mixed21): row tiles
 *               that stage V in LDS, and row tiles that read V from global memory; both -1
 *               before the plan's first fp32-residual call built those tables, and for fp32 plans.
 * Tests use it to show that a shape set reaches the paths it was chosen for. */
#define ARCTOPK_DIAG_ENCODE_TILES 9
int arctopk_diag_encode_tiles(const arctopk_plan* plan, int64_t* out, int32_t n);

/* library build identification (for smoke tests) */
const char* arctopk_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ARCTOPK_H */
