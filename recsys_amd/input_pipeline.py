"""Input pipeline: the reference's `input_fn` (fm/fm.py:106-112, deepfm/deepfm.py:60-70, xdeepfm/xdeepfm.py:101-118,
dcn/dcn.py:106-112, din/din.py:61-80) on top of librsx.so's streaming TFRecord reader (csrc/tfrecord_reader.cpp: mmap, SSE4.2 CRC, parse and batch assembly in
C++ worker threads, data-parallel sharding of the batch stream).

Order of transformations is the reference's:
    TFRecordDataset(files) -> map(parse) -> batch(bs) -> [shuffle(buffer of BATCHES)] -> prefetch -> repeat(epochs)
i.e. shuffling permutes whole batches inside a sliding window and the final partial batch of an epoch is kept.
The host half of `input_layer` (FarmHash % bucket, bucketize(log(x+shift))) runs inside the C++ parse, so the
pipeline yields `features = {'ids': int32 [B,39], 'cont_log': float32 [B,13]}` and `labels` float32 [B,1].
"""
import ctypes as C
import os
import queue
import threading

import numpy as np

from ._lib import RsxError, check, lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def read_shard(path, verify_crc=True):
    """-> (buf uint8, offsets int64 [n], lengths int64 [n]).  Raises RsxError on a corrupt record (TF: DataLossError)."""
    buf = np.fromfile(path, dtype=np.uint8)
    L = lib()
    n = L.rsx_tfrecord_index_h(_p(buf), buf.size, None, None, 0, 0)
    if n < 0:
        raise RsxError("%s: %s" % (path, L.rsx_strerror(int(n)).decode()))
    offs, lens = np.empty(n, np.int64), np.empty(n, np.int64)
    n2 = L.rsx_tfrecord_index_h(_p(buf), buf.size, _p(offs), _p(lens), n, int(verify_crc))
    if n2 < 0:
        raise RsxError("%s: %s" % (path, L.rsx_strerror(int(n2)).decode()))
    return buf, offs, lens


class _CriteoParser:
    def __init__(self, layout, threads, label_optional=False):
        self.F = layout.F
        self.threads = int(threads) | (0x10000 if label_optional else 0)    # bit 16: a missing `_c0` parses as label 0
        self.slot_src = np.array([int(c.key[2:]) for c in layout.columns], np.int32)
        self.slot_rows = np.array([c.rows for c in layout.columns], np.int32)
        bnd, off = [], [0]
        for c in layout.columns:
            bnd += list(c.boundaries or [])
            off.append(len(bnd))
        self.bnd = np.array(bnd if bnd else [0.0], np.float32)
        self.bnd_off = np.array(off, np.int32)
        shift = np.ones(13, np.float32)
        for c in layout.columns:
            if c.boundaries is not None:
                shift[int(c.key[2:]) - 1] = c.log_shift
        self.shift = shift

    def __call__(self, buf, offs, lens):
        n = len(offs)
        label = np.empty((n, 1), np.float32)
        cont = np.empty((n, 13), np.float32)
        ids = np.empty((n, self.F), np.int32)
        check(lib().rsx_criteo_parse_h(_p(buf), _p(offs), _p(lens), n, _p(self.slot_src), _p(self.slot_rows), _p(self.bnd),
                                       _p(self.bnd_off), _p(self.shift), self.F, _p(label), _p(cont), _p(ids), self.threads),
              "rsx_criteo_parse_h")
        return {"ids": ids, "cont_log": cont}, label


def log_thresholds(boundaries):
    """rsx_log_thresholds_h: per boundary b the smallest non-negative fp32 v with logf(v) >= b on THIS host's logf (verified
    per boundary).  Raises RsxError for unsorted or non-finite boundaries, or when the verification fails."""
    bd = np.ascontiguousarray(boundaries, np.float32).reshape(-1)
    thr = np.empty(bd.size, np.float32)
    check(lib().rsx_log_thresholds_h(_p(bd), int(bd.size), _p(thr)), "rsx_log_thresholds_h")
    return thr


def criteo_parse_spec(layout):
    """What the device parse (include/rsx.h rsx_parse_spec) needs of a Criteo layout, as host arrays: slot_src, slot_rows,
    thr / thr_off (the logf thresholds of every numeric slot's boundaries), shift, F, null_hash.  Raises RsxError when a slot's
    boundaries cannot be turned into thresholds."""
    cp = _CriteoParser(layout, 1, label_optional=True)
    thr, off = [], [0]
    for c in layout.columns:
        if c.boundaries is not None:
            thr += list(log_thresholds(c.boundaries))
        off.append(len(thr))
    return {"slot_src": cp.slot_src, "slot_rows": cp.slot_rows, "thr": np.array(thr if thr else [0.0], np.float32),
            "thr_off": np.array(off, np.int32), "shift": cp.shift, "F": int(layout.F),
            "null_hash": int(lib().rsx_fingerprint64_h(b"NULL", 4))}


def _batched(parse, filenames, batch_size, num_epochs, chunk_records=65536):
    """map(parse) -> batch: record streams of consecutive files are concatenated before batching, like TFRecordDataset."""
    epoch = 0
    while num_epochs < 0 or epoch < num_epochs:
        carry_f, carry_l = None, None
        for path in filenames:
            buf, offs, lens = read_shard(path)
            for s in range(0, len(offs), chunk_records):
                feats, lab = parse(buf, offs[s:s + chunk_records], lens[s:s + chunk_records])
                if carry_l is not None:
                    feats = {k: np.concatenate([carry_f[k], v]) for k, v in feats.items()}
                    lab = np.concatenate([carry_l, lab])
                n = lab.shape[0]
                full = (n // batch_size) * batch_size
                for b in range(0, full, batch_size):
                    yield {k: v[b:b + batch_size] for k, v in feats.items()}, lab[b:b + batch_size]
                carry_f = {k: v[full:] for k, v in feats.items()} if full < n else None
                carry_l = lab[full:] if full < n else None
        if carry_l is not None and carry_l.shape[0]:
            yield carry_f, carry_l                      # the final partial batch is kept
        epoch += 1


def _shuffled(it, buffer_size, seed):
    """tf.data shuffle(buffer_size) applied AFTER batch: a sliding window of whole batches."""
    rng = np.random.default_rng(seed)
    buf = []
    for x in it:
        if len(buf) < buffer_size:
            buf.append(x)
            continue
        i = int(rng.integers(0, buffer_size))
        out, buf[i] = buf[i], x
        yield out
    rng.shuffle(buf)
    yield from buf


def _prefetched(it, depth):
    """prefetch(buffer_size): a producer thread runs `it` up to `depth` batches ahead.  When the consumer stops early
    (evaluate(steps=...), predict's caller breaking out, garbage collection of the generator) the `finally` below sets
    the stop event; the producer notices within one put-timeout, closes the upstream generator (releasing the shard
    image it holds) and exits -- no thread or buffer outlives its consumer."""
    q = queue.Queue(maxsize=max(1, depth))
    end = object()
    stop = threading.Event()

    def put(x):
        while not stop.is_set():
            try:
                q.put(x, timeout=0.05)
                return True
            except queue.Full:
                continue
        return False

    def work():
        try:
            for x in it:
                if not put(x):
                    break
            else:
                put(end)
        except BaseException as e:  # surfaced in the consumer
            put(e)
        finally:
            close = getattr(it, "close", None)
            if close is not None:
                close()

    t = threading.Thread(target=work, daemon=True, name="rsx-prefetch")
    t.start()
    try:
        while True:
            x = q.get()
            if x is end:
                return
            if isinstance(x, BaseException):
                raise x
            yield x
    finally:
        stop.set()
        t.join(timeout=5.0)


def _shard_from_env(shard):
    """(rank, world) of the data-parallel job this process belongs to; explicit `shard` wins."""
    if shard is not None:
        return int(shard[0]), int(shard[1])
    return 0, 1


class _Reader:
    """Owner of one C++ streaming reader (csrc/tfrecord_reader.cpp); closed by the generator's `finally`, i.e. also when
    the consumer stops early or drops the iterator -- no thread or mapping outlives its consumer."""

    def __init__(self, handle):
        if not handle:
            raise RsxError("could not open the TFRecord reader (bad arguments)")
        self.h = C.c_void_p(handle)

    def close(self):
        if self.h is not None:
            lib().rsx_reader_close_h(self.h)
            self.h = None

    def __del__(self):
        self.close()


def _paths_array(filenames):
    arr = (C.c_char_p * len(filenames))(*[str(f).encode() for f in filenames])
    return arr


class FlatFeatures(dict):
    """The features dict of one batch whose arrays (and labels) are views of ONE flat host buffer laid out like
    estimator.PackedBatch's packing: `flat` is that buffer (np.uint8), so the Estimator wraps it instead of re-packing."""
    __slots__ = ("flat", "pack_key")       # pack_key: one hashable per stream layout (batch size, fields)


def _criteo_batches(filenames, batch_size, num_epochs, layout, threads, shard, verify_crc, queue_batches, drop_remainder):
    ps = _CriteoParser(layout, threads)
    rank, world = shard
    paths = _paths_array(filenames)
    rd = _Reader(lib().rsx_criteo_reader_open_h(paths, len(filenames), _p(ps.slot_src), _p(ps.slot_rows), _p(ps.bnd),
                                                _p(ps.bnd_off), _p(ps.shift), ps.F, int(batch_size), int(num_epochs), rank,
                                                world, int(drop_remainder), int(threads), int(verify_crc), int(queue_batches)))
    F, bs = ps.F, int(batch_size)
    # ONE flat host buffer per batch, laid out like estimator.PackedBatch packs it (label | cont_log | ids, 16-byte aligned
    # parts), so the Estimator's single H2D copy can take it as it is (PackedBatch adopts it without a copy).  The parts are
    # handed to the reader by ADDRESS (one .ctypes.data per batch instead of three data_as casts: the Python side of a batch
    # cost 70 us, more than a DeepFM step).
    o_cont = (bs * 4 + 15) & ~15
    o_ids = (o_cont + bs * 52 + 15) & ~15
    nb = o_ids + bs * F * 4
    next_h = lib().rsx_criteo_reader_next_h
    VP = C.c_void_p
    pack_key = ("criteo", bs, F)
    try:
        while True:
            flat = np.empty(nb, np.uint8)
            a = flat.ctypes.data
            n = next_h(rd.h, VP(a), VP(a + o_cont), VP(a + o_ids))
            if n == 0:
                return
            if n < 0:
                raise RsxError("%s: %s" % (filenames[0] if len(filenames) == 1 else "TFRecord stream",
                                           lib().rsx_strerror(int(n)).decode()))
            label = flat[:bs * 4].view(np.float32).reshape(bs, 1)
            cont = flat[o_cont:o_cont + bs * 52].view(np.float32).reshape(bs, 13)
            ids = flat[o_ids:o_ids + bs * F * 4].view(np.int32).reshape(bs, F)
            feats = FlatFeatures(ids=ids, cont_log=cont)
            feats.flat, feats.pack_key = flat, pack_key
            if n < bs:
                label = label[:n]
                feats = {"ids": ids[:n], "cont_log": cont[:n]}
            yield feats, label
    finally:
        rd.close()


# ---- device parse of the batch stream (opt-in; csrc/parse_records.hip) -------------------------------------------
DEVICE_PARSE_ONLY = "device parse is single-replica Criteo fm / deepfm / dcn only"
# what the stream did in this process (scripts/e2e_train_bench.py, tests): kernel launches, records, bytes shipped, batches that
# went back to the host parser
device_parse_stats = {"launches": 0, "records": 0, "bytes": 0, "fallback_batches": 0}


def check_device_parse(layout=None, world=1, model=None):
    """Raises RsxError for what the device parse does not serve: data-parallel sharding of the stream, xdeepfm.py (its linear
    part consumes the logf values themselves, which the device batches do not carry) and the uid_iid / din feature sets."""
    if int(world) > 1:
        raise RsxError("%s (the stream of %d replicas is sharded by the host reader)" % (DEVICE_PARSE_ONLY, world))
    if model is not None and str(model).split(".")[-1] not in ("fm", "deepfm", "dcn"):
        raise RsxError("%s (not %s)" % (DEVICE_PARSE_ONLY, str(model).split(".")[-1]))
    if layout is not None:
        for c in layout.columns:
            k = str(c.key)
            if not (k.startswith("_c") and k[2:].isdigit() and 1 <= int(k[2:]) <= 39):
                raise RsxError("%s (feature %r is no Criteo field)" % (DEVICE_PARSE_ONLY, k))


class DeviceFeatures(dict):
    """The device counterpart of FlatFeatures: the features dict of one batch whose `ids` (and the labels) are views of ONE
    flat DEVICE buffer in estimator.PackedBatch's own packing (label | ids, 16-byte aligned parts); `dev_flat` is that buffer
    (torch.uint8), which PackedBatch adopts without a copy.  It carries no `cont_log`."""
    __slots__ = ("dev_flat", "pack_key")


def _device_packing(rows, F):
    """-> (offset of the ids, bytes) of a [rows]-batch packed like PackedBatch packs ({'ids': int32 [rows, F]}, fp32 [rows, 1])."""
    o_ids = (rows * 4 + 15) & ~15
    return o_ids, (o_ids + rows * F * 4 + 15) & ~15


def _stream_error(filenames, code):
    return RsxError("%s: %s" % (filenames[0] if len(filenames) == 1 else "TFRecord stream", lib().rsx_strerror(int(code)).decode()))


def _map_shard(path):
    """-> (mapping uint8, payload offsets int64 [n], lengths int64 [n]): the shard memory-mapped and indexed with the framing's
    CRCs NOT verified (the device verifies them); a truncated shard raises here, as in read_shard."""
    if os.path.getsize(path) == 0:
        return np.zeros(0, np.uint8), np.zeros(0, np.int64), np.zeros(0, np.int64)
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    L = lib()
    n = L.rsx_tfrecord_index_h(_p(mm), mm.size, None, None, 0, 0)
    if n < 0:
        raise RsxError("%s: %s" % (path, L.rsx_strerror(int(n)).decode()))
    offs, lens = np.empty(n, np.int64), np.empty(n, np.int64)
    n2 = L.rsx_tfrecord_index_h(_p(mm), mm.size, _p(offs), _p(lens), n, 0)
    if n2 < 0:
        raise RsxError("%s: %s" % (path, L.rsx_strerror(int(n2)).decode()))
    return mm, offs, lens


def _batch_descriptors(filenames, batch_size, num_epochs):
    """The batch stream of the C++ reader as DESCRIPTORS: (rows, spans), a span = (mapping, offsets, lengths) of consecutive
    records of one file.  Consecutive files form one record stream, the final partial batch of an epoch is kept, num_epochs
    is honoured.  A descriptor holds its mappings alive and nothing else: a shuffle buffer of them costs no memory."""
    epoch = 0
    while num_epochs < 0 or epoch < num_epochs:
        spans, have, any_batch = [], 0, False
        for path in filenames:
            mm, offs, lens = _map_shard(path)
            s, n = 0, len(offs)
            while s < n:
                take = min(batch_size - have, n - s)
                spans.append((mm, offs[s:s + take], lens[s:s + take]))
                have, s = have + take, s + take
                if have == batch_size:
                    yield have, spans
                    spans, have, any_batch = [], 0, True
        if have:
            yield have, spans
        elif not any_batch:
            return                                      # (no record at all: an endless epoch loop would spin)
        epoch += 1


def _host_batch(spans, rows, parser, verify_crc, filenames):
    """One batch parsed on the host, what the stream falls back to when the device declined one of its records -> flat uint8 in
    the device packing.  The framing's CRCs are verified here (verify_crc); a corrupt or malformed record raises the RsxError of
    the default path."""
    L = lib()
    o_ids, nbytes = _device_packing(rows, parser.F)
    flat = np.zeros(nbytes, np.uint8)
    label = flat[:rows * 4].view(np.float32).reshape(rows, 1)
    ids = flat[o_ids:o_ids + rows * parser.F * 4].view(np.int32).reshape(rows, parser.F)
    k = 0
    for mm, offs, lens in spans:
        if verify_crc:
            for o, n in zip(offs.tolist(), lens.tolist()):
                head, rec = mm[o - 12:o], mm[o:o + n + 4]
                if int(head[8:12].view("<u4")[0]) != L.rsx_masked_crc32c_h(_p(head), 8) or \
                        int(rec[n:n + 4].copy().view("<u4")[0]) != L.rsx_masked_crc32c_h(_p(rec), n):
                    raise _stream_error(filenames, -4)
        feats, lab = parser(mm, offs, lens)
        m = len(offs)
        label[k:k + m], ids[k:k + m] = lab, feats["ids"]
        k += m
    return flat


class _DeviceParseStep:
    """The product's chunk parse: ONE H2D copy of the staged chunk (offset table, then bytes) from a pinned buffer, ONE
    rsx_criteo_parse_records launch, the status words copied back -- all on a stream of its own, waited for through an event of
    its own.  The output buffer is allocated per chunk (the yielded batches are views of it and own it); the input buffer is
    only read by the kernel and is reused after the wait."""

    def __init__(self, layout, device):
        import torch
        from ._lib import ParseSpec
        self.torch = torch
        dev = torch.device(device if device is not None else "cuda")
        self.dev = torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev
        arrays = criteo_parse_spec(layout)
        self._spec_dev = {k: torch.from_numpy(arrays[k]).to(self.dev) for k in ("slot_src", "slot_rows", "thr", "thr_off", "shift")}
        self.spec = ParseSpec()
        for k, t in self._spec_dev.items():
            setattr(self.spec, k, t.data_ptr())
        self.spec.F, self.spec.null_hash = arrays["F"], arrays["null_hash"]
        torch.cuda.synchronize(self.dev)                                 # (the spec arrays are there before the first launch)
        self.stream = torch.cuda.Stream(self.dev)
        self.event = torch.cuda.Event()
        self.pin = self.dev_in = self.status_pin = None
        self._relaxed = False

    def staging(self, nbytes):
        self._thread_setup()
        if self.pin is None or self.pin.numel() < nbytes:
            self.pin = self.torch.empty(max(nbytes, 2 * (self.pin.numel() if self.pin is not None else 0)),
                                        dtype=self.torch.uint8).pin_memory()
        return self.pin.numpy()[:nbytes]

    def _thread_setup(self):
        # this thread's copies, launches and waits must stay legal while the training thread captures a HIP graph
        if not self._relaxed:
            check(lib().rsx_thread_capture_relaxed_h(), "rsx_thread_capture_relaxed_h")
            self._relaxed = True

    def __call__(self, stage, n, tab, buf_bytes, verify_crc, rows, n_batches, stride, ids_off):
        torch = self.torch
        total = tab + buf_bytes
        self._thread_setup()
        with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
            if self.dev_in is None or self.dev_in.numel() < total:
                self.dev_in = torch.empty(max(total, 2 * (self.dev_in.numel() if self.dev_in is not None else 0)),
                                          dtype=torch.uint8, device=self.dev)
            if self.status_pin is None or self.status_pin.numel() < n:
                self.status_pin = torch.empty(max(n, 4096), dtype=torch.int32).pin_memory()
            self.dev_in[:total].copy_(self.pin[:total], non_blocking=True)
            out = torch.empty(n_batches * stride, dtype=torch.uint8, device=self.dev)
            status = torch.empty(n, dtype=torch.int32, device=self.dev)
            base = self.dev_in.data_ptr()
            check(lib().rsx_criteo_parse_records(base + tab, buf_bytes, base, base + 4 * n, n, C.byref(self.spec), int(verify_crc),
                                                 out.data_ptr(), rows, stride, ids_off, status.data_ptr(),
                                                 self.stream.cuda_stream), "rsx_criteo_parse_records")
            self.status_pin[:n].copy_(status, non_blocking=True)
            self.event.record(self.stream)
        self.event.synchronize()
        device_parse_stats["launches"] += 1
        return out, self.status_pin.numpy()[:n].copy()

    def put(self, out, off, flat):
        """A host-parsed batch into its place of the chunk's output (the fallback)."""
        torch = self.torch
        self._thread_setup()
        with torch.cuda.device(self.dev), torch.cuda.stream(self.stream):
            out[off:off + flat.size].copy_(torch.from_numpy(flat).pin_memory(), non_blocking=True)
            self.event.record(self.stream)
        self.event.synchronize()

    def close(self):
        self.pin = self.dev_in = self.status_pin = self._spec_dev = None


def _chunk_batches(chunk, F, parser, verify_crc, filenames, parse_step):
    """One chunk of descriptors (all of `rows` rows) -> its batches, in order: stage the spans (int32 rec_off [n] | int32
    rec_len [n] | the spans' bytes with their framing, each span 4-byte aligned), run the parse step, and hand out views of its
    output; a batch with a declined record is parsed on the host instead."""
    rows, nb = chunk[0][0], len(chunk)
    n = rows * nb
    o_ids, nbytes = _device_packing(rows, F)
    stride = (nbytes + 255) & ~255
    tab = (8 * n + 15) & ~15
    total, plan = tab, []
    for _, spans in chunk:
        for mm, offs, lens in spans:
            a, b = int(offs[0]) - 12, int(offs[-1] + lens[-1]) + 4
            plan.append((mm, a, b, total, offs, lens))
            total += (b - a + 3) & ~3
    staging = getattr(parse_step, "staging", None)
    stage = staging(total) if staging is not None else np.empty(total, np.uint8)
    rec_off, rec_len = stage[:4 * n].view(np.int32), stage[4 * n:8 * n].view(np.int32)
    k = 0
    for mm, a, b, dst, offs, lens in plan:
        stage[dst:dst + (b - a)] = mm[a:b]               # the ONE host copy of every byte
        m = len(offs)
        rec_off[k:k + m] = offs - (a - (dst - tab))
        rec_len[k:k + m] = np.minimum(lens, 0x7fffffff)
        k += m
    out, status = parse_step(stage, n, tab, total - tab, verify_crc, rows, nb, stride, o_ids)
    device_parse_stats["records"] += n
    device_parse_stats["bytes"] += total
    status = np.asarray(status).reshape(nb, rows)
    host = isinstance(out, np.ndarray)
    pack_key = ("criteo-device", rows, F)
    for i, (_, spans) in enumerate(chunk):
        if status[i].any():
            flat = _host_batch(spans, rows, parser, verify_crc, filenames)
            device_parse_stats["fallback_batches"] += 1
            if host:
                out[i * stride:i * stride + nbytes] = flat
            else:
                parse_step.put(out, i * stride, flat)
        flat = out[i * stride:i * stride + nbytes]
        if host:
            label = flat[:rows * 4].view(np.float32).reshape(rows, 1)
            ids = flat[o_ids:o_ids + rows * F * 4].view(np.int32).reshape(rows, F)
        else:
            import torch
            label = flat[:rows * 4].view(torch.float32).view(rows, 1)
            ids = flat[o_ids:o_ids + rows * F * 4].view(torch.int32).view(rows, F)
        feats = DeviceFeatures(ids=ids)
        feats.dev_flat, feats.pack_key = flat, pack_key
        yield feats, label


def _device_parse_batches(filenames, batch_size, num_epochs, layout, verify_crc, prefetch, chunk_batches, device, parse_step,
                          shuffle):
    """criteo_input_fn(device_parse=True): the default path's batch stream with the parse on the device.
    The stream is defined by descriptors (_batch_descriptors; `shuffle` = (buffer, seed) runs _shuffled over THEM, so the
    order of batches is the default path's).  A producer thread takes up to `chunk_batches` descriptors of equal row count (a
    partial batch is a chunk of its own), stages and parses them (_chunk_batches) and hands the batches over, at most
    `prefetch` of them ahead of the consumer.  When the consumer stops -- exhaustion, an error, close() or garbage collection of
    this generator -- the `finally` below stops the thread, which drops the descriptors (their mappings) and the parse step's
    buffers: nothing outlives the consumer."""
    F = layout.F
    parser = _CriteoParser(layout, 1)
    own_step = parse_step is None
    if own_step:
        parse_step = _DeviceParseStep(layout, device)
    chunk_batches = max(1, min(chunk_batches, prefetch))
    desc = _batch_descriptors(filenames, batch_size, num_epochs)
    if shuffle is not None:
        desc = _shuffled(desc, shuffle[0], shuffle[1])
    q = queue.Queue()
    end = object()
    stop = threading.Event()
    credits = threading.Semaphore(prefetch)            # one per batch that is parsed (or being parsed) and not yet consumed

    def acquire(k):
        for _ in range(k):
            while not credits.acquire(timeout=0.05):
                if stop.is_set():
                    return False
        return not stop.is_set()

    def work():
        try:
            pend, done = None, False
            while not stop.is_set() and not (done and pend is None):
                chunk, pend = ([pend] if pend is not None else []), None
                while not done and len(chunk) < chunk_batches:
                    d = next(desc, None)
                    if d is None:
                        done = True
                    elif chunk and d[0] != chunk[0][0]:
                        pend = d
                        break
                    else:
                        chunk.append(d)
                if not chunk:
                    continue
                if not acquire(len(chunk)):
                    return
                for b in _chunk_batches(chunk, F, parser, verify_crc, filenames, parse_step):
                    q.put(b)
                del chunk
            q.put(end)
        except BaseException as e:  # surfaced in the consumer
            q.put(e)
        finally:
            desc.close()
            if own_step:
                parse_step.close()

    t = threading.Thread(target=work, daemon=True, name="rsx-device-parse")
    t.start()
    try:
        while True:
            x = q.get()
            if x is end:
                return
            if isinstance(x, BaseException):
                raise x
            credits.release()
            flat = x[0].dev_flat
            if not isinstance(flat, np.ndarray):
                # allocated on the producer's stream, about to be read on the consumer's: the allocator must not hand the memory
                # out again before that stream is done with it (PackedBatch records the stream that adopts it as well)
                import torch
                flat.record_stream(torch.cuda.current_stream(flat.device))
            yield x
    finally:
        stop.set()
        t.join(timeout=5.0)
        while not q.empty():                            # batches parsed ahead go with the consumer
            q.get_nowait()


RSX_SHARD_TAIL = 2      # include/rsx.h: value of drop_remainder


def _shard_tail(shard_tail, num_epochs, need_shuffle):
    """Sharded EVALUATION has no collective inside its loop, so the ranks need not run equal step counts: with shard_tail=True
    (what run_main's eval input_fns pass) the leftover batches of the last round and the final partial batch are delivered
    too (csrc/tfrecord_reader.cpp RSX_SHARD_TAIL) -- together the ranks then evaluate exactly the examples a single replica
    would.  An explicit opt-in (default False): a data-parallel TRAIN stream that happened to be built with
    num_epochs=1 and no shuffle must keep complete rounds only, or its ranks run unequal step counts and deadlock in the
    step's collectives."""
    return RSX_SHARD_TAIL if shard_tail else 0


def criteo_input_fn(filenames, batch_size, num_epochs=-1, need_shuffle=False, num_parallel=8, layout=None,
                    shuffle_buffer=1000, prefetch=16, seed=0, shard=None, verify_crc=True, shard_tail=False,
                    device_parse=False, device=None, parse_chunk_batches=8, parse_step=None):
    """fm/fm.py:106-112.  Returns an iterator of (features, labels).
    shard=(rank, world): this replica's share of the batch stream (see csrc/tfrecord_reader.cpp); each replica then
    shuffles its own sub-stream with its own seed.  `prefetch` = batches the C++ reader keeps in flight.
    shard_tail (default False; evaluation passes True): see _shard_tail.
    device_parse (default False: nothing changes): the shards' raw bytes go to `device` and rsx_criteo_parse_records parses
    `parse_chunk_batches` batches per launch (see _device_parse_batches); the batches are device tensors, `ids` and labels
    only (no `cont_log`), in the same order and with the same bits as the default path.  Single replica only.
    parse_step: the chunk parse as a callable (tests run the stream on numpy buffers with the kernel's host twin)."""
    if layout is None:
        from .feature_columns import CriteoLayout, build_feature_columns
        layout = CriteoLayout.from_columns(build_feature_columns(16)[1])
    rank, world = _shard_from_env(shard)
    if device_parse:
        check_device_parse(layout=layout, world=world)
        return _device_parse_batches(list(filenames), int(batch_size), int(num_epochs), layout, bool(verify_crc),
                                     max(1, int(prefetch)), max(1, int(parse_chunk_batches)), device, parse_step,
                                     (shuffle_buffer, seed) if need_shuffle else None)
    it = _criteo_batches(list(filenames), batch_size, num_epochs, layout, num_parallel, (rank, world), verify_crc,
                         max(2, prefetch), drop_remainder=_shard_tail(shard_tail, num_epochs, need_shuffle) if world > 1 else 0)
    if need_shuffle:
        it = _shuffled(it, shuffle_buffer, seed + 7919 * rank)
    return it


def din_input_fn(filenames, batch_size, num_epochs=-1, need_shuffle=False, num_parallel=6, hist_len=100,
                 shuffle_buffer=1000, prefetch=16, seed=0, ids_int32=False, shard=None, verify_crc=True, shard_tail=False):
    """din/din.py:61-80: features {'i_id','i_cate' int64 [B]; 'u_iid_seq','u_icat_seq' int64 [B,P]}, labels int64 [B].
    ids_int32: narrow the id features to int32 on the HOST (the device kernels index with int32; like the Criteo parse,
    which emits int32 row ids) so that the training step has no per-feature cast launches."""
    P, bs = int(hist_len), int(batch_size)
    rank, world = _shard_from_env(shard)
    filenames = list(filenames)

    def gen():
        paths = _paths_array(filenames)
        tail = _shard_tail(shard_tail, num_epochs, need_shuffle) if world > 1 else 0
        rd = _Reader(lib().rsx_din_reader_open_h(paths, len(filenames), P, bs, int(num_epochs), rank, world, tail,
                                                 int(num_parallel), int(verify_crc), max(2, int(prefetch))))
        try:
            while True:
                lab, iid, icat = (np.empty(bs, np.int64) for _ in range(3))
                hi, hc = np.empty((bs, P), np.int64), np.empty((bs, P), np.int64)
                n = lib().rsx_din_reader_next_h(rd.h, _p(lab), _p(iid), _p(icat), _p(hi), _p(hc))
                if n == 0:
                    return
                if n < 0:
                    raise RsxError("DIN TFRecord stream: %s" % lib().rsx_strerror(int(n)).decode())
                if n < bs:
                    lab, iid, icat, hi, hc = lab[:n], iid[:n], icat[:n], hi[:n], hc[:n]
                # (id 0 is the history padding (din/din.py:56-57,107) AND an ordinary row for the target lookups, as in the
                # reference: the device side keys the padding entries to a dummy row, so a target id 0 trains normally)
                # Negative ids would index in front of the tables (tf.gather raises InvalidArgument on CPU): refuse them here.
                if min(int(iid.min()), int(icat.min()), int(hi.min()), int(hc.min())) < 0:
                    raise RsxError("DIN TFRecord stream: negative id in i_id / i_cate / u_iid_seq / u_icat_seq")
                if ids_int32:
                    iid, icat, hi, hc = (x.astype(np.int32) for x in (iid, icat, hi, hc))
                yield {"i_id": iid, "i_cate": icat, "u_iid_seq": hi, "u_icat_seq": hc}, lab
        finally:
            rd.close()

    it = gen()
    if need_shuffle:
        it = _shuffled(it, shuffle_buffer, seed + 7919 * rank)
    return it


def uid_iid_input_fn(filenames, batch_size=32, num_epochs=-1, need_shuffle=False, layout=None, shuffle_buffer=100, seed=0):
    """deepfm/deepfm.py:53-70 AS COMMITTED: records {label int64, u_id int64, i_id int64} -> features {'ids' int32 [B,2]}
    (hashed on the host like the Criteo categorical fields), labels float32 [B].  Small utility path (the BASELINE configs
    are the Criteo marriage): whole shards are indexed and parsed at once."""
    names = (C.c_char_p * 3)(b"label", b"u_id", b"i_id")

    def gen():
        epoch = 0
        while num_epochs < 0 or epoch < num_epochs:
            carry = None
            for path in filenames:
                buf, offs, lens = read_shard(path)
                n = len(offs)
                out = np.empty((3, n), np.int64)
                check(lib().rsx_int64_features_parse_h(_p(buf), _p(offs), _p(lens), n, names, 3, _p(out), 4),
                      "rsx_int64_features_parse_h")
                if carry is not None:
                    out = np.concatenate([carry, out], 1)
                full = (out.shape[1] // batch_size) * batch_size
                for b in range(0, full, batch_size):
                    sl = out[:, b:b + batch_size]
                    yield {"ids": layout.transform_int64({"u_id": sl[1], "i_id": sl[2]})}, sl[0].astype(np.float32)
                carry = out[:, full:] if full < out.shape[1] else None
            if carry is not None and carry.shape[1]:
                yield {"ids": layout.transform_int64({"u_id": carry[1], "i_id": carry[2]})}, carry[0].astype(np.float32)
            epoch += 1

    it = gen()
    if need_shuffle:
        it = _shuffled(it, shuffle_buffer, seed)
    return it


# ---- serialized tf.train.Example entry -------------------------------------------------------------
def _pack_serialized(serialized):
    """list of bytes -> (buf uint8, offsets int64 [n], lengths int64 [n])."""
    lens = np.fromiter((len(x) for x in serialized), np.int64, len(serialized))
    offs = np.zeros(len(serialized), np.int64)
    if len(serialized) > 1:
        np.cumsum(lens[:-1], out=offs[1:])
    buf = np.frombuffer(b"".join(serialized), np.uint8)
    if buf.size == 0:
        buf = np.zeros(1, np.uint8)
    return buf, offs, lens


def parse_criteo_examples(serialized, layout, threads=1):
    """What the exported model's parsing signature does with the strings a serving client sends
    (deepfm/grpc_client.py:50-76 builds one serialized tf.train.Example per request row; the SavedModel parses them with
    the script's feature_description, deepfm/deepfm.py:213-233): -> (features, labels) like one input_fn batch.
    The label feature `_c0` is optional here (serving requests carry none)."""
    if not len(serialized):
        raise ValueError("no examples")
    buf, offs, lens = _pack_serialized(serialized)
    feats, label = _CriteoParser(layout, threads, label_optional=True)(buf, offs, lens)
    return feats, label


def parse_din_examples(serialized, hist_len=100, ids_int32=True):
    """din/din.py:44-57 parse spec applied to in-memory serialized Examples."""
    if not len(serialized):
        raise ValueError("no examples")
    buf, offs, lens = _pack_serialized(serialized)
    n, P = len(serialized), int(hist_len)
    lab, iid, icat = (np.empty(n, np.int64) for _ in range(3))
    hi, hc = np.empty((n, P), np.int64), np.empty((n, P), np.int64)
    check(lib().rsx_din_parse_h(_p(buf), _p(offs), _p(lens), n, P, _p(lab), _p(iid), _p(icat), _p(hi), _p(hc), 1),
          "rsx_din_parse_h")
    if ids_int32:
        iid, icat, hi, hc = (x.astype(np.int32) for x in (iid, icat, hi, hc))
    return {"i_id": iid, "i_cate": icat, "u_iid_seq": hi, "u_icat_seq": hc}, lab


# ---- synthetic shard writers (the reference's sample shard is a missing blob) ------------
def write_criteo_shard(path, label, cont, cat):
    """label [n] f32, cont [n,13] f32, cat: n lists of 26 bytes values ('NULL' entries are omitted on disk)."""
    from .synthetic import pack_cat
    label = np.ascontiguousarray(label, np.float32).reshape(-1)
    cont = np.ascontiguousarray(cont, np.float32)
    buf, offs = pack_cat(cat)
    L = lib()
    need = L.rsx_criteo_encode_h(_p(label), _p(cont), _p(buf), _p(offs), len(label), None, 0)
    cap = -int(need)
    out = np.empty(cap, np.uint8)
    n = L.rsx_criteo_encode_h(_p(label), _p(cont), _p(buf), _p(offs), len(label), _p(out), cap)
    if n < 0:
        raise RsxError("rsx_criteo_encode_h failed (%d)" % n)
    out[:n].tofile(path)
    return int(n)


def write_din_shard(path, batch, keep_padding=False):
    lab, iid, icat = (np.ascontiguousarray(batch[k], np.int64) for k in ("label", "i_id", "i_cate"))
    hi, hc = np.ascontiguousarray(batch["u_iid_seq"], np.int64), np.ascontiguousarray(batch["u_icat_seq"], np.int64)
    L = lib()
    n_ex, P = hi.shape
    need = L.rsx_din_encode_h(_p(lab), _p(iid), _p(icat), _p(hi), _p(hc), n_ex, P, int(keep_padding), None, 0)
    cap = -int(need)
    out = np.empty(cap, np.uint8)
    n = L.rsx_din_encode_h(_p(lab), _p(iid), _p(icat), _p(hi), _p(hc), n_ex, P, int(keep_padding), _p(out), cap)
    if n < 0:
        raise RsxError("rsx_din_encode_h failed (%d)" % n)
    out[:n].tofile(path)
    return int(n)
