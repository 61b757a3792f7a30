"""Differential run of the sharded cytosine and lMHL reports: one library per process (EPIHIP_LIB selects it), one JSON of
case -> digest per run; two libraries behave alike where their JSON files are identical.  Needs the GPU.

    EPIHIP_LIB=/path/to/parent/libepihip.so python scratch/shard_refactor_diff.py parent.json
    python scratch/shard_refactor_diff.py new.json
    cmp parent.json new.json

World size 1 throughout, shared tiles forced.  Cases, over the batches of tests/test_gpu_sharded.py (_case) and its two seam
batches: the native reports (epi_batch_*_report_sharded on a library communicator with 5 forced shared tiles) -- thresholded CG
twice, un-thresholded CX twice, lMHL "Zz" with two clamps, "[[" and "ZzXxHh", a plain report behind them; the two-step
reports (set_shared / report / finish_shared through the engine's methods with the first tiles of the range as shared keys) on
all three slab kinds; a too-small pool (EPIHIP_CX_SLOT=0, CG then CHH: the deferred report reruns its first half); the
refusals -- unsorted rows, keys not increasing, NULL slabs, fused slabs on a batch that needs the two-kernel path, a second
half without a first, NULL arguments and mismatched engines of the sharded entry points.  A digest covers every column's
bytes, the return code and error text, last_exchange_bytes, and the live device allocations before and after the step."""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import epialleler_amd as ea  # noqa: E402
from epialleler_amd import _lib, distributed as D  # noqa: E402
import synth_np  # noqa: E402
import test_gpu_sharded as TS  # noqa: E402

RESULTS = {}
lib = _lib.load()


def allocations():
    n, nbytes = C.c_int64(0), C.c_int64(0)
    lib.epi_device_allocations(C.byref(n), C.byref(nbytes))
    return [n.value, nbytes.value]


def digest(rep):
    h = hashlib.sha256()
    for k, v in rep.items():
        v = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
        h.update(k.encode())
        h.update(repr((v.dtype.str, v.shape)).encode())
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def case(name, fn):
    assert name not in RESULTS, name
    before = allocations()
    try:
        out = fn()
    except Exception as e:                                          # the message is part of the behaviour
        out = "%s: %s" % (type(e).__name__, e)
    RESULTS[name] = {"result": out, "allocations": [before, allocations()]}


def rc(code):
    msg = lib.epi_last_error()
    return "ok" if code == 0 else "%d: %s" % (code, msg.decode("utf-8", "replace") if msg else "")


def columns(block_names):
    return {k: blk[i] for blk, names in block_names for i, k in enumerate(names)}


def as_bam(t):
    return ea.ProcessedBam.from_arrays(t["xm"], t["off"], t["rname"], t["strand"], t["start"])


def native_cases(tag, t):
    shard = as_bam(t)
    eng = D.HipShardEngine(shard).attach_comm(test_shared=5)
    with_bytes = lambda rep: [digest(rep), rep.nrow, eng.last_exchange_bytes]
    for thr, rctx in ((True, "CG"), (False, "CX")):
        for k in range(2):                                           # (the second call: remembered plan, deferred synchronisation)
            case("%s native %s #%d" % (tag, rctx, k),
                 lambda: with_bytes(D.sharded_cytosine_report(eng, threshold_reads=thr, report_context=rctx)))
    for ctx, hmax in (("Zz", 0), ("Zz", 2), ("[[", 0), ("ZzXxHh", 0), ("Zz", 0)):
        case("%s native lMHL %s hmax=%d%s" % (tag, ctx, hmax, " again" if "%s native lMHL %s hmax=%d" % (tag, ctx, hmax) in RESULTS else ""),
             lambda: with_bytes(D.sharded_mhl_report(eng, ctx, hmax, 0, 0.1)))
    case(tag + " plain behind native", lambda: digest(ea.generateCytosineReport(shard, threshold_reads=True)))
    case(tag + " plain lMHL behind native", lambda: digest(ea.generateMhlReport(shard)))
    eng.close_comm()
    shard.close()


def first_keys(eng, kind, n, ctx="Z"):
    first, last = eng.key_range(kind, ctx)
    return np.array([k for k in range(first, first + n) if (k >> 32) == (first >> 32) and k <= last], dtype=np.int64)


def two_step_cases(tag, t):
    shard = as_bam(t)
    eng = D.HipShardEngine(shard)
    c = ea.CONTEXT_TO_BASES["CG"]
    thr = (c["ctx_meth"], c["ctx_unmeth"], c["ooctx_meth"], c["ooctx_unmeth"], 2, 0.5, 0.1)

    def cx(ctx, fused):
        keys = first_keys(eng, "cx", 4, ctx)
        owned = (np.arange(keys.size) % 2 == 0).astype(np.int32)     # (tiles of other owners stay out of the table)
        slab = eng.cx_accumulate_fused(thr, ctx, keys, owned) if fused else eng.cx_accumulate(None, ctx, keys, owned)
        return [int(slab.abs().sum()), digest(columns([(eng.cx_finish(ctx), D.CX_COLUMNS)]))]

    def mhl(ctx, fused):
        keys = first_keys(eng, "mhlf" if fused else "mhl", 3)
        cnt, sums = eng.mhl_accumulate(ctx, 0, 0, 0.1, keys, np.ones(keys.size, np.int32), fused=fused)
        icols, dcols = eng.mhl_finish()
        return [int(cnt.abs().sum()), int(sums.abs().sum()), digest(columns([(icols, D.MHL_COLUMNS[:5]), (dcols, D.MHL_COLUMNS[5:])]))]

    for k in range(2):
        case("%s two-step CG fused thresholding #%d" % (tag, k), lambda: cx("Z", True))
        case("%s two-step CX #%d" % (tag, k), lambda: cx("ZXH", False))
    case(tag + " two-step lMHL two-kernel", lambda: mhl("Zz", False))
    case(tag + " two-step lMHL six letters", lambda: mhl("ZzXxHh", False))
    if eng.mhl_fused_ok("Zz"):
        case(tag + " two-step lMHL one-pass", lambda: mhl("Zz", True))
    case(tag + " plain behind two-step", lambda: digest(ea.generateCytosineReport(shard, threshold_reads=True)))
    shard.close()


def pool_retry_cases():
    os.environ["EPIHIP_CX_SLOT"] = "0"
    lib.epi_options_reload()
    try:
        shard = as_bam(synth_np.generate(n_total=60000, read_len=300, n_chr=2))
        eng = D.HipShardEngine(shard).attach_comm(test_shared=5)
        for k, rctx in enumerate(("CG", "CG", "CHH", "CHH")):
            case("pool retry %s #%d" % (rctx, k), lambda: (lambda rep: [digest(rep), rep.nrow, eng.last_exchange_bytes])(
                D.sharded_cytosine_report(eng, threshold_reads=False, report_context=rctx, gather=False)))
        eng.close_comm()
        shard.close()
    finally:
        del os.environ["EPIHIP_CX_SLOT"]
        lib.epi_options_reload()


def error_cases():
    t = TS._case("wgs")
    shard = as_bam(t)
    b = shard.batch()
    eng = D.HipShardEngine(shard).attach_comm(test_shared=5)
    nrow = C.c_int64(7)
    keys = first_keys(eng, "cx", 3)
    owned = np.ones(3, np.int32)
    kp, op = C.c_void_p(keys.ctypes.data), C.c_void_p(owned.ctypes.data)
    down = np.ascontiguousarray(keys[::-1])
    twice = np.ascontiguousarray(keys[[0, 1, 1]])
    T = lib.epi_cx_tile_positions(b"Z")
    slab = torch.zeros(3 * 16 * T, dtype=torch.int32, device="cuda")
    sums = torch.zeros(3 * 6 * 1024, dtype=torch.int64, device="cuda")
    sp, qp = C.c_void_p(slab.data_ptr()), C.c_void_p(sums.data_ptr())
    state = lambda code: [rc(code), nrow.value]

    case("finish without a first half: CX", lambda: state(lib.epi_batch_cx_finish_shared(b, b"Z", None, C.byref(nrow))))
    case("finish without a first half: lMHL", lambda: state(lib.epi_batch_mhl_finish_shared(b, None, C.byref(nrow))))
    case("finish: NULL arguments", lambda: [rc(lib.epi_batch_cx_finish_shared(b, None, None, C.byref(nrow))),
                                            rc(lib.epi_batch_cx_finish_shared(None, b"Z", None, C.byref(nrow))),
                                            rc(lib.epi_batch_mhl_finish_shared(b, None, None))])
    for name, ks in (("decreasing", down), ("repeated", twice)):
        p = C.c_void_p(ks.ctypes.data)
        case("keys %s: CX" % name, lambda: rc(lib.epi_batch_cx_set_shared(b, p, op, 3, sp)))
        case("keys %s: lMHL" % name, lambda: rc(lib.epi_batch_mhl_set_shared(b, p, op, 3, sp, qp)))
        case("keys %s: lMHL one-pass" % name, lambda: rc(lib.epi_batch_mhl_set_shared_fused(b, p, op, 3, sp, qp)))
        case("keys %s: plain report behind" % name, lambda: digest(ea.generateCytosineReport(shard, threshold_reads=False)))
    case("NULL slab: CX", lambda: rc(lib.epi_batch_cx_set_shared(b, kp, op, 3, None)))
    case("NULL slab: lMHL counters", lambda: rc(lib.epi_batch_mhl_set_shared(b, kp, op, 3, None, qp)))
    case("NULL slab: lMHL sums", lambda: rc(lib.epi_batch_mhl_set_shared(b, kp, op, 3, sp, None)))
    case("NULL slab: lMHL one-pass", lambda: rc(lib.epi_batch_mhl_set_shared_fused(b, kp, op, 3, sp, None)))
    case("NULL keys, NULL batch, negative count", lambda: [rc(lib.epi_batch_cx_set_shared(b, None, op, 3, sp)),
                                                           rc(lib.epi_batch_mhl_set_shared(b, kp, None, 3, sp, qp)),
                                                           rc(lib.epi_batch_cx_set_shared(None, kp, op, 3, sp)),
                                                           rc(lib.epi_batch_mhl_set_shared(None, None, None, 0, None, None)),
                                                           rc(lib.epi_batch_cx_set_shared(b, kp, op, -1, sp))])
    case("plain report behind the refusals", lambda: digest(ea.generateCytosineReport(shard, threshold_reads=True)))
    case("CX slab attached, finish of the other report", lambda: [
        rc(lib.epi_batch_cx_set_shared(b, kp, op, 3, sp)), state(lib.epi_batch_cx_report_dev(b, None, b"Z", None, C.byref(nrow))),
        state(lib.epi_batch_mhl_finish_shared(b, None, C.byref(nrow))), state(lib.epi_batch_cx_finish_shared(b, b"Z", None, C.byref(nrow))),
        state(lib.epi_batch_cx_finish_shared(b, b"Z", None, C.byref(nrow))), rc(lib.epi_batch_cx_set_shared(b, None, None, 0, None))])
    case("sharded entry points: NULL arguments", lambda: [
        state(lib.epi_batch_cytosine_report_sharded(None, eng.comm, None, None, None, None, 0, 0.0, 0.0, None, b"Z", None, None, C.byref(nrow))),
        state(lib.epi_batch_cytosine_report_sharded(b, None, None, None, None, None, 0, 0.0, 0.0, None, b"Z", None, None, C.byref(nrow))),
        state(lib.epi_batch_cytosine_report_sharded(b, eng.comm, None, None, None, None, 0, 0.0, 0.0, None, None, None, None, C.byref(nrow))),
        rc(lib.epi_batch_cytosine_report_sharded(b, eng.comm, None, None, None, None, 0, 0.0, 0.0, None, b"Z", None, None, None)),
        state(lib.epi_batch_mhl_report_sharded(None, eng.comm, b"Zz", 0, 0, 0.1, None, C.byref(nrow))),
        state(lib.epi_batch_mhl_report_sharded(b, eng.comm, None, 0, 0, 0.1, None, C.byref(nrow))),
        rc(lib.epi_batch_mhl_report_sharded(b, eng.comm, b"Zz", 0, 0, 0.1, None, None))])
    case("sharded cytosine report: thresholding context without its partner", lambda: [
        state(lib.epi_batch_cytosine_report_sharded(b, eng.comm, b"Z", None, None, None, 2, 0.5, 0.1, None, b"Z", None, None, C.byref(nrow))),
        int(lib.epi_comm_last_exchange_bytes(eng.comm))])
    case("native report behind the refusals", lambda: [digest(D.sharded_cytosine_report(eng, report_context="CG")), eng.last_exchange_bytes])
    eng.close_comm()
    shard.close()

    # the one-pass kernel's slabs on a batch that needs the two-kernel path (a row longer than the kernel takes)
    long_t = synth_np.with_long_tail(TS._case("wgs"), 61, 9000, first=7)
    shard = as_bam(long_t)
    eng = D.HipShardEngine(shard)
    case("long rows: one-pass kernel allowed", lambda: eng.mhl_fused_ok("Zz"))

    def fused_on_long():
        keys = first_keys(eng, "mhlf", 3)
        try:
            eng.mhl_accumulate("Zz", 0, 0, 0.1, keys, np.ones(keys.size, np.int32), fused=True)
            return "accepted"
        finally:
            lib.epi_batch_mhl_set_shared(shard.batch(), None, None, 0, None, None)

    case("fused slabs, two-kernel batch", fused_on_long)
    case("fused slabs, two-kernel batch: finish", lambda: state(lib.epi_batch_mhl_finish_shared(shard.batch(), None, C.byref(nrow))))
    case("fused slabs, two-kernel batch: plain lMHL behind", lambda: digest(ea.generateMhlReport(shard)))
    shard.close()

    # unsorted rows
    u = {k: v.copy() for k, v in TS._case("wgs").items()}
    u["start"][100], u["start"][101] = u["start"][101] + 50, u["start"][100]
    shard = as_bam(u)
    eng = D.HipShardEngine(shard).attach_comm(test_shared=5)
    case("unsorted: native CX", lambda: digest(D.sharded_cytosine_report(eng, report_context="CG")))
    case("unsorted: native lMHL", lambda: digest(D.sharded_mhl_report(eng, "Zz", 0, 0, 0.1)))
    case("unsorted: native lMHL six letters", lambda: digest(D.sharded_mhl_report(eng, "ZzXxHh", 0, 0, 0.1)))
    case("unsorted: exchange bytes", lambda: int(lib.epi_comm_last_exchange_bytes(eng.comm)))
    eng.close_comm()
    eng2 = D.HipShardEngine(shard)
    case("unsorted: key range", lambda: eng2.key_range())
    shard.close()


if __name__ == "__main__":
    print("library:", _lib.LIB_PATH)
    for name in ("wgs", "amplicon", "mixed", "wgs_tail"):
        native_cases(name, TS._case(name))
        two_step_cases(name, TS._case(name))
    for name in ("empty", "one_tile"):
        native_cases(name, TS._seam_case(name))
    pool_retry_cases()
    error_cases()
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(RESULTS, f, indent=0, sort_keys=True)
    errors = sum(1 for v in RESULTS.values() if isinstance(v["result"], str) and ": " in v["result"])
    print("%d cases (%d of them Python-level errors) -> %s" % (len(RESULTS), errors, sys.argv[1]))
