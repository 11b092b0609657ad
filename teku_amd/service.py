"""GPU-aware signature verification service.

Mirrors statetransition/.../validation/signatures/
AggregatingSignatureVerificationService.java: callers submit
(public-key lists, messages, signatures) tasks and get a future; worker
threads drain the queue into batches of up to max_batch_size tasks
(waitForBatch, l.164-179) and verify each batch with one randomized
BLS.batchVerify (batchVerifySignatures, l.188-205).

The difference is the failure path.  The reference, when a batch fails,
halves it recursively down to min_batch_size_to_split tasks and then verifies
each remaining task alone (l.211-227, splitTasks l.230-233): O(bad * log n)
extra batch verifications, each a full GPU round trip.  Here the batch and its
failure path are one call, tbls_batch_verify_each: when the batch fails, the
library settles every set's fastAggregateVerify verdict from the batch's own
Miller work on the same devices (group tests over 256- and 16-set groups, then
single sets), and a task is valid iff all its sets are
(BLSSignatureVerifier.SIMPLE.verify -> BLS.batchVerify over the task's sets,
BLSSignatureVerifier.java:27-43, which is the same boolean with overwhelming
probability).  `split_fallback=True` restores the reference's halving, for
comparison; a custom batch_fn keeps the batch + per-set pass of round 4.

Defaults follow the GPU (round 6): one worker thread per device, as the
reference sizes its workers to the host's cores (numThreads,
AggregatingSignatureVerificationService.java:68-69, 121-132; P2PConfig
.java:42-43), and a large max batch (the device wants >= 16k sets; the
reference default is 250).  Each worker's batch is placed by the library
(tb_plan.h place_plan): with more tasks waiting in the queue the worker
passes n_gpus = 1, so concurrent batches land on distinct devices, one each;
a batch that leaves the queue empty may take every idle device, down to 4,096
sets per device on an idle node (the latency knee).

Host glue (round 6): a task's future is a TaskFuture (the verdict is one
attribute store, the waiting callers woken once per batch, instead of a
concurrent.futures.Future's lock and notify per task: 15 ms of 16,384
set_result calls), and the batch is marshalled straight into the C set
array.

Grouped batches (`group_messages=True`, off by default): attestations of one
slot sign the same AttestationData, so a gossip batch carries few distinct
messages.  The happy path then calls tbls_batch_verify_grouped -- one hash and
one pairing per distinct message where the library finds that grouping pays,
the same verdict as the ungrouped batch -- and a batch that fails it goes to
tbls_batch_verify_each as before, which gives the per-set verdicts and settles.
With `group_settle=True` as well (off by default) the batch is one call,
tbls_batch_verify_each_grouped: a grouped batch that fails settles its per-set
verdicts from the grouped pass's own work, with no second staging, decoding or
hashing of the sets.

Hash-point memo (`hash_memo_rows=N`, off by default): gossip delivers a slot's
attestations over seconds, in batches of a few hundred sets that sign the same
few signing roots, so batch after batch would hash the same 32 bytes again.
With N > 0 start() configures the library's per-device memo of N rows
(tbls_msg_memo_configure): every later batch, its settling included, hashes
only the messages no earlier batch left on the device.  Verdicts are
unchanged; metrics() reports the memo's counters.

Semantics kept from the reference: a full queue completes the future
exceptionally with ServiceCapacityExceededException (verify, l.143-152);
verify() before start() raises (assertIsRunning); a one-task failed batch is
that task's verdict (l.208-210).  A task whose list sizes differ completes
exceptionally with BlsException (BLS.batchVerify throws, BLS.java:235-237).
"""

import queue
import threading
from operator import attrgetter
from typing import Callable, List, Optional, Sequence

from . import bls as _bls
from . import native
from .synth import SetArray, fast_multipliers

DEFAULT_MIN_BATCH_SIZE_TO_SPLIT = 25  # AggregatingSignatureVerificationService.java:42
DEFAULT_MAX_BATCH_SIZE = 16384
DEFAULT_QUEUE_CAPACITY = 65536


class ServiceCapacityExceededException(RuntimeError):
    """infrastructure/async/.../ServiceCapacityExceededException."""


class TaskFuture:
    """The result of one verify() call: SafeFuture<Boolean> in the reference
    (AggregatingSignatureVerificationService.SignatureTask.result, l.241),
    with the subset of concurrent.futures.Future's interface the callers use
    (result, exception, done, add_done_callback, set_result, set_exception).
    Completion is an attribute store; waiters sleep on one condition shared
    by every future of a service and are woken once per batch
    (complete_all), so completing a 16,384-task batch costs ~16,384 stores
    instead of 16,384 lock / notify rounds."""

    __slots__ = ("_cond", "_state", "_value", "_callbacks")
    _PENDING, _DONE, _FAILED = 0, 1, 2

    def __init__(self, cond: Optional[threading.Condition] = None):
        self._cond = cond if cond is not None else _SHARED_COND
        self._state = TaskFuture._PENDING
        self._value = None
        self._callbacks = None

    def done(self) -> bool:
        return self._state != TaskFuture._PENDING

    def _wait(self, timeout):
        if self._state == TaskFuture._PENDING:
            with self._cond:
                if not self._cond.wait_for(self.done, timeout):
                    raise TimeoutError("signature verification still pending")

    def result(self, timeout: Optional[float] = None):
        self._wait(timeout)
        if self._state == TaskFuture._FAILED:
            raise self._value
        return self._value

    def exception(self, timeout: Optional[float] = None):
        self._wait(timeout)
        return self._value if self._state == TaskFuture._FAILED else None

    def add_done_callback(self, fn):
        with self._cond:
            if self._state == TaskFuture._PENDING:
                self._callbacks = (self._callbacks or []) + [fn]
                return
        fn(self)

    def _settle(self, state, value):
        self._value = value
        self._state = state

    def _run_callbacks(self):
        cbs, self._callbacks = self._callbacks, None
        for fn in cbs or ():
            fn(self)

    def set_result(self, value):
        with self._cond:
            self._settle(TaskFuture._DONE, value)
            self._cond.notify_all()
        self._run_callbacks()

    def set_exception(self, exc):
        with self._cond:
            self._settle(TaskFuture._FAILED, exc)
            self._cond.notify_all()
        self._run_callbacks()

    @staticmethod
    def complete_all(futures: Sequence["TaskFuture"], values: Sequence[bool]):
        """Complete a batch's futures with one wake-up per condition they
        wait on (normally one: the service's)."""
        if not futures:
            return
        conds = set(map(_get_cond, futures))
        for c in conds:
            c.acquire()
        try:
            for f, v in zip(futures, values):
                f._value = v
                f._state = TaskFuture._DONE
            for c in conds:
                c.notify_all()
        finally:
            for c in conds:
                c.release()
        if any(map(_get_callbacks, futures)):
            for f in futures:
                if f._callbacks:
                    f._run_callbacks()


_SHARED_COND = threading.Condition()  # futures made outside a service
_get_result = attrgetter("result")
_get_cond = attrgetter("_cond")
_get_callbacks = attrgetter("_callbacks")


class SignatureTask:
    """AggregatingSignatureVerificationService.SignatureTask (l.236-258): the
    task's signature sets as (pk_blob, n_pks, msg, sig96) tuples."""

    __slots__ = ("sets", "result")

    def __init__(self, sets, cond: Optional[threading.Condition] = None):
        self.sets = sets
        self.result = TaskFuture(cond)


def _set_tuple(pks, msg, sig):
    blob = b"".join(bytes(p.to_bytes_compressed() if hasattr(p, "to_bytes_compressed") else p) for p in pks)
    sigb = bytes(sig.to_bytes_compressed() if hasattr(sig, "to_bytes_compressed") else sig)
    return (blob, len(pks), bytes(msg), sigb)


def _hip_batch(sets, timing=None) -> bool:
    rands = fast_multipliers(len(sets))  # BlstBLS12381.java:191-195 (nextBatchRandomMultiplier), one CSPRNG call
    try:
        return SetArray.from_tuples(sets).batch_verify(rands, timing=timing)
    except ValueError:  # an empty key list in the batch: false, then settled per task (_verify)
        return False


def _hip_each(sets) -> List[bool]:
    return SetArray.from_tuples(sets).verify_each()


def _hip_batch_each(sets, n_gpus=0, timing=None):
    """(batch verdict, per-set verdicts) in one device call (tbls_batch_verify_each)."""
    return SetArray.from_tuples(sets).batch_verify_each(fast_multipliers(len(sets)), n_gpus=n_gpus, timing=timing)


def _hip_batch_grouped(sets, n_gpus=0, timing=None, force=False) -> bool:
    """The batch verdict over message groups (tbls_batch_verify_grouped)."""
    try:
        return SetArray.from_tuples(sets).batch_verify_grouped(fast_multipliers(len(sets)), n_gpus=n_gpus, force=force, timing=timing)
    except ValueError:  # an empty key list in the batch: false, then settled per set
        return False


def _hip_batch_each_grouped(sets, n_gpus=0, timing=None, force=False):
    """(batch verdict, per-set verdicts) over message groups in one device call (tbls_batch_verify_each_grouped)."""
    return SetArray.from_tuples(sets).batch_verify_each_grouped(fast_multipliers(len(sets)), n_gpus=n_gpus, force=force, timing=timing)


def default_num_threads() -> int:
    """One worker per device (the library's device count), 1 without one."""
    try:
        return max(1, native.lib().tbls_device_count())
    except Exception:  # no device: the custom-backend (CPU) services
        return 1


class AggregatingSignatureVerificationService:
    def __init__(
        self,
        num_threads: Optional[int] = None,
        queue_capacity: int = DEFAULT_QUEUE_CAPACITY,
        max_batch_size: int = DEFAULT_MAX_BATCH_SIZE,
        min_batch_size_to_split: int = DEFAULT_MIN_BATCH_SIZE_TO_SPLIT,
        split_fallback: bool = False,
        batch_fn: Optional[Callable[[Sequence], bool]] = None,
        each_fn: Optional[Callable[[Sequence], List[bool]]] = None,
        batch_each_fn: Optional[Callable] = None,
        group_messages: bool = False,
        group_force: bool = False,
        batch_grouped_fn: Optional[Callable] = None,
        group_settle: bool = False,
        batch_each_grouped_fn: Optional[Callable] = None,
        hash_memo_rows: int = 0,
    ):
        """num_threads: workers (default: one per device for the device
        backend, 1 for a custom batch_fn).  batch_each_fn(sets, n_gpus,
        timing) -> (ok, per-set verdicts) replaces the device call of the
        default path (tbls_batch_verify_each) -- e.g. a placement simulator
        in the CPU tests.  group_messages: the default path first calls
        batch_grouped_fn(sets, n_gpus, timing) -> ok (tbls_batch_verify_grouped)
        and only a failed batch goes on to batch_each_fn; group_force: the
        library groups whenever a message repeats (TBLS_GROUP_FORCE), not
        only where its thresholds say that grouping pays.  group_settle
        (with group_messages): the batch is one call of
        batch_each_grouped_fn(sets, n_gpus, timing) -> (ok, per-set verdicts)
        (tbls_batch_verify_each_grouped), which settles a failed grouped
        batch from the grouped pass.  hash_memo_rows: rows per device of the
        library's hash-point memo, configured by start() when not 0 (process
        state: it stays configured for every caller of the library)."""
        if num_threads is None:
            num_threads = default_num_threads() if batch_fn is None else 1
        self.num_threads = max(1, num_threads)
        self.max_batch_size = max(1, max_batch_size)
        self.min_batch_size_to_split = min_batch_size_to_split
        self.split_fallback = split_fallback
        self._batch_fn = batch_fn or _hip_batch
        self._each_fn = each_fn or _hip_each
        self._batch_each_fn = batch_each_fn or _hip_batch_each
        self.group_messages = group_messages
        if batch_grouped_fn is None:
            batch_grouped_fn = (lambda sets, n_gpus, timing: _hip_batch_grouped(sets, n_gpus, timing, True)) if group_force else _hip_batch_grouped
        self._batch_grouped_fn = batch_grouped_fn
        self.group_settle = group_settle
        self.hash_memo_rows = int(hash_memo_rows)
        if batch_each_grouped_fn is None:
            batch_each_grouped_fn = ((lambda sets, n_gpus, timing: _hip_batch_each_grouped(sets, n_gpus, timing, True)) if group_force
                                     else _hip_batch_each_grouped)
        self._batch_each_grouped_fn = batch_each_grouped_fn
        self.batch_signature_tasks: "queue.Queue[SignatureTask]" = queue.Queue(maxsize=queue_capacity)
        self._cond = threading.Condition()  # every task future of this service waits on it
        self.n_gpus_log: List[int] = []  # the n_gpus each device batch was placed with
        self._running = False
        self._threads: List[threading.Thread] = []
        # metrics (signature_verifications_{batch_count,task_count}_total, batch_size histogram)
        self.batch_count = 0
        self.task_count = 0
        self.batch_sizes: List[int] = []
        self.device_passes = 0
        # device metrics beside the reference's: per batch
        # pass, the library's tbls_timing (kernel pipeline ms over the devices,
        # host ms API entry -> verdict, devices used)
        self.sets_verified = 0
        self.device_ms_total = 0.0
        self.host_ms_total = 0.0
        self.last_batch_timing: Optional[dict] = None
        # group_messages: batches that went through the grouped entry, their sets and distinct messages
        self.grouped_batches = 0
        self.grouped_sets = 0
        self.grouped_messages = 0

    # -- Service lifecycle -------------------------------------------------
    def start(self):
        if self.hash_memo_rows:
            from . import bls

            bls.msg_memo_configure(self.hash_memo_rows)
        self._running = True
        for i in range(self.num_threads):
            t = threading.Thread(target=self._run, name=f"sigverify-{i}", daemon=True)
            t.start()
            self._threads.append(t)
        return self

    def stop(self):
        self._running = False
        for t in self._threads:
            t.join()
        self._threads = []

    def is_running(self) -> bool:
        return self._running

    # -- SignatureVerificationService.verify -----------------------------------
    def verify(self, public_keys, message, signature) -> TaskFuture:
        """verify(List<BLSPublicKey>, Bytes, BLSSignature) (l.129-133)."""
        return self.verify_many([public_keys], [message], [signature])

    def verify_many(self, public_keys, messages, signatures) -> TaskFuture:
        """verify(List<List<BLSPublicKey>>, List<Bytes>, List<BLSSignature>) (l.135-153)."""
        if not self._running:
            raise RuntimeError("Service must be running to execute action 'verify'")
        if not (len(public_keys) == len(messages) == len(signatures)):
            f = TaskFuture(self._cond)
            f.set_exception(_bls.BlsException("Different collection sizes"))
            return f
        task = SignatureTask([_set_tuple(p, m, s) for p, m, s in zip(public_keys, messages, signatures)], self._cond)
        try:
            self.batch_signature_tasks.put_nowait(task)
        except queue.Full:
            task.result.set_exception(ServiceCapacityExceededException("Failed to process signature, queue is full."))
        return task.result

    def queue_size(self) -> int:
        return self.batch_signature_tasks.qsize()

    # -- worker ---------------------------------------------------------------
    def _run(self):
        while self._running:
            tasks = self._wait_for_batch()
            if tasks:
                self.batch_verify_signatures(tasks)

    def _wait_for_batch(self) -> List[SignatureTask]:
        tasks = []
        try:
            tasks.append(self.batch_signature_tasks.get(timeout=0.05))
        except queue.Empty:
            return tasks
        while len(tasks) < self.max_batch_size:
            try:
                tasks.append(self.batch_signature_tasks.get_nowait())
            except queue.Empty:
                break
        return tasks

    def batch_verify_signatures(self, tasks: List[SignatureTask]):
        self.batch_count += 1
        self.task_count += len(tasks)
        self.batch_sizes.append(len(tasks))
        try:
            self._verify(tasks)
        except Exception as e:  # device error: fail every pending future loudly
            for t in tasks:
                if not t.result.done():
                    t.result.set_exception(e)

    def _verify(self, tasks: List[SignatureTask]):
        empty = [t for t in tasks if not t.sets]  # SIMPLE.verify of zero sets -> false (BLS.java:240-241)
        for t in empty:
            t.result.set_result(False)
        if empty:
            tasks = [t for t in tasks if t.sets]
        if not tasks:
            return
        all_sets = [s for t in tasks for s in t.sets]
        if self._batch_fn is _hip_batch and not self.split_fallback:
            # more tasks waiting: this batch takes one device, so the next
            # worker's batch gets another; an empty queue lets the library
            # shard it over the idle devices (tbls_place_plan)
            n_gpus = 1 if self.batch_signature_tasks.qsize() > 0 else 0
            self.n_gpus_log.append(n_gpus)
            self.device_passes += 1
            t = native.TblsTiming()
            ok, verdicts = False, None
            if self.group_messages:
                self.grouped_batches += 1
                self.grouped_sets += len(all_sets)
                self.grouped_messages += len({s[2] for s in all_sets})
                if self.group_settle:  # the batch and its failure path in the one grouped call
                    ok, verdicts = self._batch_each_grouped_fn(all_sets, n_gpus, t)
                else:
                    ok = self._batch_grouped_fn(all_sets, n_gpus, t)
                    if not ok:  # per-set verdicts, settled as without the flag
                        self.device_passes += 1
                        self.device_ms_total += t.device_ms
                        self.host_ms_total += t.total_ms
            if not ok and verdicts is None:
                ok, verdicts = self._batch_each_fn(all_sets, n_gpus, t)
            self.sets_verified += len(all_sets)
            self.device_ms_total += t.device_ms
            self.host_ms_total += t.total_ms
            self.last_batch_timing = {"sets": len(all_sets), "device_ms": t.device_ms, "total_ms": t.total_ms, "n_devices": t.n_devices,
                                      "settled": not ok}
            futs = list(map(_get_result, tasks))
            if ok:
                vals = [True] * len(tasks)
            elif len(all_sets) == len(tasks):  # one set per task (gossip)
                vals = verdicts
            else:
                vals, k = [], 0
                for task in tasks:
                    n = len(task.sets)
                    vals.append(all(verdicts[k : k + n]))
                    k += n
            TaskFuture.complete_all(futs, vals)
            return
        self.device_passes += 1
        if self._batch_timed(all_sets):
            for t in tasks:
                t.result.set_result(True)
            return
        if len(tasks) == 1 and not self.split_fallback:
            tasks[0].result.set_result(False)  # l.208-210
            return
        if self.split_fallback:
            self._split(tasks)
            return
        self.device_passes += 1
        verdicts = self._each_fn(all_sets)
        k = 0
        for t in tasks:
            n = len(t.sets)
            t.result.set_result(all(verdicts[k : k + n]))
            k += n

    def _batch_timed(self, sets) -> bool:
        """One batch pass, with the device timing when the default batch
        function runs (a custom batch_fn is timed on the host only)."""
        if self._batch_fn is not _hip_batch:
            return self._batch_fn(sets)
        t = native.TblsTiming()
        ok = _hip_batch(sets, timing=t)
        self.sets_verified += len(sets)
        self.device_ms_total += t.device_ms
        self.host_ms_total += t.total_ms
        self.last_batch_timing = {"sets": len(sets), "device_ms": t.device_ms, "total_ms": t.total_ms, "n_devices": t.n_devices}
        return ok

    def metrics(self) -> dict:
        """The reference's executor metrics (AggregatingSignatureVerificationService.java:76-98:
        signature_verifications_queue_size, _batch_count_total, _task_count_total,
        _batch_size histogram) and the device's: sets verified per second of
        kernel time (summed over devices) and of host wall time, the last
        batch's timing."""
        memo = {}
        if self.hash_memo_rows:  # (pairs from rows, messages hashed, flushes, rows in use), process-wide
            from . import bls

            memo = {"hash_memo": bls.msg_memo_stats()}
        return {
            **memo,
            "signature_verifications_queue_size": self.queue_size(),
            "signature_verifications_batch_count_total": self.batch_count,
            "signature_verifications_task_count_total": self.task_count,
            "signature_verifications_batch_size": list(self.batch_sizes),
            "device_passes_total": self.device_passes,
            "device_sets_verified_total": self.sets_verified,
            "device_kernel_ms_total": self.device_ms_total,
            "device_sets_per_s": self.sets_verified / (self.device_ms_total * 1e-3) if self.device_ms_total > 0 else None,
            "host_sets_per_s": self.sets_verified / (self.host_ms_total * 1e-3) if self.host_ms_total > 0 else None,
            "last_batch": self.last_batch_timing,
            "grouped_batches_total": self.grouped_batches,
            "grouped_sets_per_message": self.grouped_sets / self.grouped_messages if self.grouped_messages else None,
        }

    def _split(self, tasks: List[SignatureTask]):
        """The reference's fallback (l.208-227): halve down to
        min_batch_size_to_split tasks, then each task alone."""
        if len(tasks) == 1:
            tasks[0].result.set_result(False)
        elif len(tasks) >= self.min_batch_size_to_split:
            half = (len(tasks) + 1) // 2
            for part in (tasks[:half], tasks[half:]):
                self.device_passes += 1
                sets = [s for t in part for s in t.sets]
                if self._batch_fn(sets):
                    for t in part:
                        t.result.set_result(True)
                else:
                    self._split(part)
        else:
            for t in tasks:
                self.device_passes += 1
                t.result.set_result(all(self._each_fn(t.sets)))
