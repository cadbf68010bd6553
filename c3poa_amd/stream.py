"""Streaming driver of the CLI: native FASTQ reader -> GPU batches -> native writer.

Replaces the read loop / mp.Pool dispatch / per-group temp files of /root/reference/C3POa.py:236-271 with a software
pipeline that keeps every GPU busy: while batch i runs on the device (its worker thread blocks in c3_batch_run, which
releases the GIL), other threads parse batch i+1, copy it to the device (c3_batch_stage) and write the records of batch i-1.  No per-read Python objects are created for sequences or qualities: the
reader fills page-locked SoA buffers that c3_batch_upload copies by DMA and c3_write_group slices for the subread file.

The reference's -g (group size) only decides how reads are partitioned into <splint>/tmp<k>/ directories that are
concatenated and deleted at the end (C3POa.py:259-271); here a GPU batch is max(-g, GPU_BATCH_READS) reads (or
C3_GPU_BATCH_READS when set) and records are appended to the final files directly (same output tree, no double write).
"""
import contextlib
import dataclasses
import gzip
import os
import queue
import shutil
import sys
import threading
import time

import numpy as np

from . import _lib

GPU_BATCH_READS = 131072         # enough reads to fill 256 CUs many times over (bench.py runs 100 000 per step)
HANDLES_PER_GPU = 1              # measured: two handles per GPU make the persistent kernels fight for CUs (0.55x)
GPU_BATCH_BASES = 1 << 30        # bound on host/device memory per batch
READERS_PER_GPU = 2              # byte-range readers (parser threads) per GPU worker
MIN_RANGE_BYTES = 256 << 20      # no point in cutting small inputs


def _is_bgzf(path):
    """what c3_reader_open looks at: the first gzip member opens with the BGZF size subfield 'BC'"""
    with open(path, "rb") as fh:
        hd = fh.read(18)
    return len(hd) == 18 and hd[:3] == b"\x1f\x8b\x08" and bool(hd[3] & 4) and hd[10:16] == b"\x06\x00BC\x02\x00"


def count_reads(path, lencutoff, assigner):
    """first pass of C3POa.py:200-207 + the bookkeeping of bin/preprocess.py:36-44: (reads passing the length cut-off,
    short reads, reads without a splint).  Names-only parse, native lookups."""
    rd = _lib.Reader(path, n_sets=1, names_only=True)
    total = short = assigned = 0
    while True:
        hb = rd.next(GPU_BATCH_READS, lencutoff, GPU_BATCH_BASES)
        short += hb.n_short
        if hb.n == 0:
            break
        total += hb.n
        assigned += assigner.batch(hb)[2]
    rd.close()
    return total, short, total - assigned


class DictAssigner:
    """adapter for callers that hold the reference's adapter_dict {name: [splint, strand]} (tests, stage seams)"""

    def __init__(self, adapter_dict, splint_names):
        self.d, self.sid_of = adapter_dict, {n: i for i, n in enumerate(splint_names)}

    def batch(self, hb):
        sid = np.full(hb.n, -1, dtype=np.int16)
        st = bytearray(b"?" * hb.n)
        k = 0
        for i, name in enumerate(hb.names()):
            ad = self.d.get(name)
            if ad:
                sid[i] = self.sid_of[ad[0]]; st[i] = 45 if ad[1] == "-" else 43; k += 1
        return sid, bytes(st), k


_KEPT = []
# Ownership of the host buffers is explicit: a reader fills buffer set j only after taking j from its free list, and the
# writer puts j back once the group has been written (device threads finish out of order, so a counting semaphore over
# round-robin sets would let a reader overwrite a set a lagging device still holds).  Result buffers follow the same
# rule: one object per batch in flight, returned by the writer.  Pipeline.release is that rule.
N_SETS = 5                                          # (a sixth set would cover every stage at once; it costs 20 % more page-locked memory and start-up time for a stall that the timeline does not show)


@dataclasses.dataclass(frozen=True)
class Options:
    """every switch of a run, read ONCE from args and the environment: nothing below looks at either again"""
    reads: str; out_path: str; lencutoff: int; mdistcutoff: int; zero: bool; zero_max_cells: int
    compress: bool; bgzf: bool; qv: bool; emit_gpu: bool; inflate_gpu: bool; parse_gpu: bool; gunzip_gpu: bool
    bam: bool
    batch_reads: int; batch_fixed: bool; n_work: int; readers_per_gpu: int; min_range: int
    devices: tuple                                  # worker -> physical device

    @classmethod
    def read(cls, args, n_dev, env=os.environ):
        # C3_GPU_BATCH_READS overrides the GPU batch size (tests drive the multi-batch pipeline with small inputs)
        gpu_batch = int(env.get("C3_GPU_BATCH_READS", "0"))
        n_work = n_dev * int(env.get("C3_HANDLES_PER_GPU", HANDLES_PER_GPU))
        devices = [w % n_dev for w in range(n_work)]
        if env.get("C3_DEVICE_MAP"):                # test hook: worker -> physical device (two workers on one GPU)
            dmap = [int(x) for x in env["C3_DEVICE_MAP"].split(",")]
            devices = [dmap[d % len(dmap)] for d in devices]
        return cls(
            reads=args.reads, out_path=args.out_path, lencutoff=args.lencutoff, mdistcutoff=args.mdistcutoff, zero=bool(getattr(args, "zero", True)),
            zero_max_cells=int(getattr(args, "zero_max_cells", _lib.ZERO_MAX_CELLS)), compress=bool(getattr(args, "compress_output", False)),
            # --bgzf (implies -co): every writer call compresses its text on the GPU (k_bgzf) and appends BGZF members to <path>.gz;
            # no uncompressed file is created and there is no pass after the run
            bgzf=bool(getattr(args, "bgzf", False)),
            # --consensus-fastq: per-base QVs on the GPU (STAGE_QV) and R2C2_Consensus.fastq beside the FASTA
            qv=bool(getattr(args, "consensus_fastq", False)),
            # --emit gpu: the records of every batch are formatted on the GPU while it is resident (k_emit; with --bgzf compressed there
            # as well) and the writer only appends the finished streams
            emit_gpu=getattr(args, "emit", "host") == "gpu",
            # --bam (needs --emit gpu): the records leave the device as unaligned BAM, always BGZF (k_bamout, k_bgzf), into
            # R2C2_Consensus.bam and R2C2_Subreads.bam; QVs, when computed, are the consensus qualities
            bam=bool(getattr(args, "bam", False)),
            inflate_gpu=getattr(args, "inflate", "host") == "gpu", parse_gpu=getattr(args, "parse", "host") == "gpu",
            # --gunzip gpu: a plain gzip input is inflated by the k_gunzip kernels instead of one zlib stream (needs --inflate gpu)
            gunzip_gpu=getattr(args, "gunzip", "host") == "gpu",
            batch_reads=gpu_batch if gpu_batch > 0 else max(int(args.groupSize), GPU_BATCH_READS), batch_fixed=gpu_batch > 0, n_work=n_work,
            readers_per_gpu=max(1, int(env.get("C3_READERS_PER_GPU", READERS_PER_GPU))), min_range=int(env.get("C3_MIN_RANGE_BYTES", MIN_RANGE_BYTES)),
            devices=tuple(devices))


class OutputTree:
    """the files of a run, <out_path><splint>/R2C2_Consensus.fasta and R2C2_Subreads.fastq (and R2C2_Consensus.fastq with QVs), written
    as X, or as X.gz with --bgzf: which exist, what a run does to them before and after.  No thread, no handle.  finder_psl: the
    fused mode's PSL, collected in finder_psl + ".part" while the run lasts."""

    def __init__(self, out_path, splint_names, bgzf=False, compress=False, qv=False, finder_psl=None, bam=False):
        self.out_path, self.names, self.bgzf, self.compress, self.qv, self.finder_psl = out_path, list(splint_names), bgzf, compress, qv, finder_psl
        self.bam_head = None                        # --bam: the header member every .bam begins with
        self.bam = bam                              # --bam: R2C2_Consensus.bam and R2C2_Subreads.bam and nothing else (bgzf, compress and qv name no file)
        self.cons_paths = [out_path + n + "/R2C2_Consensus.fasta" for n in self.names]
        self.sub_paths = [out_path + n + "/R2C2_Subreads.fastq" for n in self.names]
        self.fq_paths = [out_path + n + "/R2C2_Consensus.fastq" for n in self.names] if qv else []
        gz = ".gz" if bgzf else ""
        self.cons_w, self.sub_w, self.fq_w = ([p + gz for p in ps] for ps in (self.cons_paths, self.sub_paths, self.fq_paths))
        # stream s * K + kind of c3_batch_emit_fetch -> its file
        self.bam_w = [(out_path + n + "/R2C2_Consensus.bam", out_path + n + "/R2C2_Subreads.bam") for n in self.names] if bam else []
        self.emit_paths = [p for k in range(len(self.names)) for p in self.written(k)]
        self.gz_made = []                           # --bgzf: the .gz files of this run (each gets the EOF member at the end)

    def written(self, k):                           # the files the writers append to for splint k
        if self.bam:
            return self.bam_w[k]
        return (self.cons_w[k], self.sub_w[k]) + ((self.fq_w[k],) if self.qv else ())

    def prepare(self, used):
        """empty files for the splints in `used` (all of them in fused mode), no stale counterpart beside them"""
        if self.finder_psl:
            used = set(self.names)                  # not known yet: directories of splints nobody used are removed at the end
            open(self.finder_psl + ".part", "w").close()
        for k, n in enumerate(self.names):
            if n in used:
                os.makedirs(self.out_path + n, exist_ok=True)
                if self.bam:
                    self.prepare_bam(k)
                    continue
                for p in self.written(k):           # "w+" semantics of cat_files (C3POa.py:88-92)
                    open(p, "w").close()
                    stale = p[:-3] if self.bgzf else p + ".gz"
                    if os.path.exists(stale):
                        os.remove(stale)
                    if self.bgzf:
                        self.gz_made.append(p)

    def prepare_bam(self, k):
        """--bam: each file of splint k starts with the BAM header as one BGZF member (host code: no worker runs yet); no text
        counterpart, plain or .gz, stays beside them"""
        if self.bam_head is None:
            self.bam_head = _lib.bgzf_compress_host(_lib.bam_out_header())
        for p in self.bam_w[k]:
            with open(p, "wb") as fh:
                fh.write(self.bam_head)
            self.gz_made.append(p)
        d = self.out_path + self.names[k] + "/"
        for stale in ("R2C2_Consensus.fasta", "R2C2_Subreads.fastq", "R2C2_Consensus.fastq"):
            for q in (d + stale, d + stale + ".gz"):
                if os.path.exists(q):
                    os.remove(q)

    def finish(self, seen=None):
        """after the last writer.  seen: the splints that were hit (fused mode), else None"""
        unused = len(self.bam_head or b"")                          # --bam: an unused file holds only its header member
        if seen is not None:
            os.replace(self.finder_psl + ".part", self.finder_psl)  # a rerun finds the PSL and takes the two-pass route
            for k, n in enumerate(self.names):
                if n not in seen:                                   # adapter_set of bin/preprocess.py:34,43 = splints that were hit
                    for p in self.written(k):                       # (before the EOF members: an unused .gz is still empty)
                        if os.path.exists(p) and os.stat(p).st_size == unused:
                            os.remove(p)
                    with contextlib.suppress(OSError):
                        os.rmdir(self.out_path + n)
        if self.bgzf or self.bam:                                   # every writer is done: the EOF member ends each file
            for p in self.gz_made:
                if os.path.exists(p):
                    with open(p, "ab") as fh:
                        fh.write(_lib.BGZF_EOF)
        elif self.compress:                                         # -co (C3POa.py:88-90)
            for p in self.cons_paths + self.sub_paths + self.fq_paths:
                if os.path.exists(p):
                    with open(p, "rb") as src, gzip.open(p + ".gz", "wb", compresslevel=6) as dst:
                        shutil.copyfileobj(src, dst, 1 << 24)
                    os.remove(p)


def open_readers(opt):
    """(readers, n_ranges).  The input is cut into contiguous BYTE RANGES, one native reader (thread) per range, READERS_PER_GPU
    ranges per worker: every GPU parses its own part of the file ("contiguous file ranges per GPU"), and one parser
    thread (~2 GB/s of FASTQ) no longer caps the node.  All workers append to the same output files (c3_write_group
    reserves each group's byte range under a lock): no per-group temp files, no merge pass (C3POa.py:259-271 concatenates
    <splint>/tmp<k>/ directories in glob order -- the reference's record order is arbitrary as well; here it is the
    round-robin order of the ranges, and the file order itself with a single range)."""
    size = os.path.getsize(opt.reads)
    zipped = str(opt.reads).endswith((".gz", ".bam"))
    splittable = not zipped and size > 0            # (BGZF, BAM included, cannot be entered in the middle)
    n_ranges = max(1, min(opt.n_work * opt.readers_per_gpu, size // max(opt.min_range, 1))) if splittable else 1
    # --inflate gpu: the (single, whole-file) reader of a .gz or .bam input inflates its BGZF stretches with k_inflate on worker
    # 0's device instead of zlib threads; any other gzip file has no member sizes to split on and is read as before
    inflate_dev, parse_dev, gunzip_dev = None, False, False
    if opt.inflate_gpu and zipped:
        if opt.gunzip_gpu and str(opt.reads).endswith(".gz") and not _is_bgzf(opt.reads):
            # --gunzip gpu: plain gzip inflated in parallel on worker 0's device (k_gunzip); with --parse gpu its text stays there
            # for k_fastq, as a BGZF file's does
            inflate_dev, parse_dev, gunzip_dev = opt.devices[0], opt.parse_gpu, True
        elif _is_bgzf(opt.reads):
            # --parse gpu: ... and its records are found there too (k_fastq; k_bam for a .bam); only the finished arrays come to the host
            inflate_dev, parse_dev = opt.devices[0], opt.parse_gpu
        else:
            print("C3POa: --inflate gpu: %s is gzip but not BGZF (no member size in front); only BGZF can be inflated on the GPU, the file is read as before" % opt.reads, file=sys.stderr)

    def whole_file():
        return [_lib.Reader(opt.reads, n_sets=N_SETS, inflate_device=inflate_dev, parse_device=parse_dev, gunzip_device=gunzip_dev)], 1
    if n_ranges == 1:
        return whole_file()
    cuts = [size * k // n_ranges for k in range(n_ranges)] + [-1]
    readers = [_lib.Reader(opt.reads, n_sets=N_SETS, byte_range=(cuts[k], cuts[k + 1])) for k in range(n_ranges)]
    if any(r.range_lost() for r in readers):
        # a range with bytes but no 4-line record start (multi-line FASTQ, which mm.fastx_read accepts): such a file cannot be
        # entered in the middle -- its records would be dropped silently -- so ONE reader takes the whole file
        for r in readers:
            r.close()
        return whole_file()
    return readers, n_ranges


class Timers:
    """the stats of a run (the dict `t`) and their lock: every write goes through add, put or a `with timers(key):`"""

    def __init__(self, n_ranges, emit_gpu):
        self.lock, self.start = threading.Lock(), time.perf_counter()
        self.t = dict(parse=0.0, assign=0.0, upload=0.0, upload_dev=0.0, run=0.0, run_c=0.0, run_dev=0.0, alloc=0.0, fetch=0.0, snapshot=0.0, write=0.0, wait_in=0.0, wait_out=0.0,
                      setup=0.0, close=0.0, scan=0.0, reads=0, batches=0, short=0, assigned=0, ranges=n_ranges)
        if emit_gpu:                                # kernel times of k_emit (and k_bgzf inside the fetch), summed over the batches
            self.t.update(emit_len=0.0, emit_scan=0.0, emit_write=0.0, emit_bgzf=0.0, emit_call=0.0, emit_bytes=0, emit_records=0)

    def add(self, **kv):                            # t[k] += v
        with self.lock:
            for k, v in kv.items():
                self.t[k] += v

    def put(self, *marks, **kv):                    # t[k] = v, and t[m] = seconds since the pipeline started for each mark m
        with self.lock:
            self.t.update(kv, **{m: time.perf_counter() - self.start for m in marks})

    @contextlib.contextmanager
    def __call__(self, key):                        # with timers(key): ...   adds the seconds spent inside
        t0 = time.perf_counter()
        try:
            yield
        finally:
            self.add(**{key: time.perf_counter() - t0})


class Batch:
    """one batch on its way parsed -> to_fetch -> to_write; each stage fills in its fields.  hb names the reader set it lies in (range_index,
    set_index); rb (ResultBuffers) and eb (EmitBuffers) are taken by the fetch stage; Pipeline.release gives all three back"""
    __slots__ = ("hb", "sid", "st", "shape", "n_streams", "res", "buf", "coff", "qv", "rb", "eb", "so")

    def __init__(self, hb, sid, st):
        self.hb, self.sid, self.st = hb, sid, st
        self.shape = self.n_streams = self.res = self.buf = self.coff = self.qv = self.rb = self.eb = self.so = None


class Pipeline:
    """reader stage (one thread per range) -> parsed -> device stage (one per worker) -> to_fetch -> fetch stage -> to_write ->
    writer stage, and the pools the batches borrow their buffers from.

    THE HANDLE PROTOCOL: what the stages call on a handle (_lib.Handle, looked up at call time; the stand-ins FakeHandle of
    tests/test_stream_pipeline_cpu.py and InstantHandle of tools/host_ceiling.py implement the part their runs reach)
      Handle(device=, mdistcutoff=, zero=, zero_max_cells=), set_splints(splints), close()
      upload_host(hb, strands, splint_ids) | stage_host(hb, strands, splint_ids), then commit()
      run(); run(qv=True) with --consensus-fastq only: a stand-in without QVs takes no argument
      last_timing: a dict with ms_pack and ms_total; ms_wall and ms_alloc are optional
      results_snapshot() -> shape; one snapshot per handle, the next waits for the fetch of this one (fetched[w])
      results_fetch(rb, shape[, with_cons=False]) -> (res, buf, coff) | results_fetch_qv(rb, shape) -> (res, buf, coff, qv)
      --emit gpu: emit_snapshot(hb, zero, bgzf, qv) -> n_streams (--bam: emit_snapshot(hb, zero, True, qv, bam=True)); emit_fetch(eb, n_streams) -> (eb, stream_off); emit_timing() -> dict
      fused finder: scan_splints() -> (table, splint_ids, strands); assign(splint_ids, strands); cfg.conk_match"""

    def __init__(self, opt, tree, readers, splints, assigner, timers):
        self.opt, self.tree, self.readers, self.splints, self.assigner, self.timers = opt, tree, readers, splints, assigner, timers
        self.fused, n_ranges, n_work = assigner is None, len(readers), opt.n_work
        # same page-locked footprint per GPU as one reader
        self.batch_reads = opt.batch_reads if opt.batch_fixed else max(opt.batch_reads // max(1, n_ranges // n_work), 16384)
        self.free_sets = [queue.Queue() for _ in range(n_ranges)]
        for fs in self.free_sets:
            for j in range(N_SETS):
                fs.put(j)
        self.free_results, self.free_emit = queue.Queue(), queue.Queue()
        self.result_bufs = [_lib.ResultBuffers() for _k in range(4 * n_work + 2)]  # run -> fetch -> (queue of 2) -> write: four batches per worker can hold one
        # --emit gpu: page-locked arenas of the streams, grow-only, owned like the result buffers
        self.emit_bufs = [_lib.EmitBuffers() for _k in range(4 * n_work)] if opt.emit_gpu else []
        for pool, bufs in ((self.free_results, self.result_bufs), (self.free_emit, self.emit_bufs)):
            for x in bufs:
                pool.put(x)
        self.parsed = [queue.Queue(maxsize=1) for _ in range(n_ranges)]
        self.to_write = [queue.Queue(maxsize=2) for _ in range(n_work)]
        self.to_fetch = [queue.Queue(maxsize=1) for _ in range(n_work)]
        self.fetched = [threading.Event() for _ in range(n_work)]
        for ev in self.fetched:
            ev.set()
        self.live = [[k for k in range(n_ranges) if k % n_work == w] for w in range(n_work)]       # the ranges each worker serves, round-robin
        self.rr, self.handles = [0] * n_work, [None] * n_work
        self.seen, self.errors, self.psl_lock = set(), [], threading.Lock()

    def release(self, *batches):
        """the buffers a batch holds go back to their owners: the reader set to its range's free list, rb and eb to their pools"""
        for b in batches:
            if b is not None:
                k, j, rb, eb = b.hb.range_index, b.hb.set_index, b.rb, b.eb
                b.hb = b.res = b.buf = b.coff = b.qv = b.rb = b.eb = b.so = None  # no view of a buffer outlives its return
                for pool, x in ((self.free_results, rb), (self.free_emit, eb), (self.free_sets[k], j)):
                    if x is not None:
                        pool.put(x)

    def take(self, w, block=True):
        """next parsed batch of worker w's ranges in STRICT round-robin (the record order of a run does not depend on
        thread timing); None when all ranges are exhausted; block=False raises queue.Empty when the range whose turn it is
        has nothing ready"""
        live = self.live[w]
        with self.timers("wait_in"):
            while live:
                k = live[self.rr[w] % len(live)]
                item = self.parsed[k].get() if block else self.parsed[k].get_nowait()
                if item is None:
                    i = live.index(k)
                    live.remove(k)
                    self.rr[w] = i                                  # the next range moved into this position
                    continue
                self.rr[w] = (live.index(k) + 1) % len(live)
                return item
            return None

    def reader_stage(self, k):                      # parse + splint/strand lookup of range k, ahead of its GPU
        rd, opt = self.readers[k], self.opt
        ks = None                                   # the buffer set this thread holds and has not handed on
        try:
            while not self.errors:
                ks = self.free_sets[k].get()
                t0 = time.perf_counter()
                hb = rd.next(self.batch_reads, opt.lencutoff, GPU_BATCH_BASES, set_index=ks)
                t1 = time.perf_counter()
                if rd.noqual():
                    # C3POa.py:167 averages ord(q) - 33 over the read's quality string and racon is run with -q 5: records
                    # without qualities cannot go through the reference either (it raises on qual = None).  An ordinary
                    # exception, so that it lands in `errors` and run() re-raises it (SystemExit would end this thread silently)
                    raise _lib.C3Error("C3POa: %s holds records without base qualities (FASTA); the consensus caller needs FASTQ" % opt.reads)
                if hb.n == 0:
                    self.timers.add(short=hb.n_short)
                    self.free_sets[k].put(ks); ks = None
                    break
                sid, st, na = (np.zeros(hb.n, dtype=np.int16), b"?" * hb.n, 0) if self.fused else self.assigner.batch(hb)
                self.timers.add(parse=t1 - t0, assign=time.perf_counter() - t1, reads=hb.n, batches=1, short=hb.n_short, assigned=na)
                hb.range_index = k
                self.parsed[k].put(Batch(hb, sid, st)); ks = None
        except BaseException as e:                  # noqa: BLE001 -- re-raised by the caller's thread
            self.errors.append(e)
        finally:                                    # whatever happened: the worker of this range must see the end marker
            if ks is not None:
                self.free_sets[k].put(ks)
            self.parsed[k].put(None)

    def find_splints(self, h, b):                   # fused mode: splint / strand of the resident batch from the GPU finder
        names = self.tree.names
        with self.timers("scan"):
            tab, b.sid, b.st = h.scan_splints()
            h.assign(b.sid, b.st)
            with self.psl_lock:
                na = _lib.write_splint_psl(b.hb, tab, b.sid, b.st, names, [len(s) for s in self.splints], h.cfg.conk_match, self.tree.finder_psl + ".part")
                self.seen.update(names[x] for x in np.unique(b.sid[b.sid >= 0]))
        self.timers.add(assigned=na)

    def run_batch(self, w, h, b):
        """c3_batch_run of the resident batch b, its snapshot, and b goes to the fetch stage.  False: an error elsewhere has
        ended the run and b stays with the caller"""
        opt = self.opt
        t1 = time.perf_counter()
        h.run(qv=True) if opt.qv else h.run()
        t2 = time.perf_counter()
        lt = h.last_timing
        dev = dict(upload_dev=lt["ms_pack"] * 1e-3, run_dev=lt["ms_total"] * 1e-3, run_c=lt.get("ms_wall", 0.0) * 1e-3, alloc=lt.get("ms_alloc", 0.0) * 1e-3)
        # results: frozen on the device here (c3_batch_results_snapshot, ~0.3 ms); the worker's fetch thread copies them to
        # the host while this thread commits and runs the next batch.  One snapshot per handle: wait for the previous fetch
        # (it started a whole batch ago)
        self.fetched[w].wait()
        if self.errors:
            return False
        self.fetched[w].clear()
        b.shape = h.results_snapshot()
        if opt.bam:                                 # BAM records, always as BGZF members
            b.n_streams = h.emit_snapshot(b.hb, opt.zero, True, opt.qv, bam=True)
        else:
            b.n_streams = h.emit_snapshot(b.hb, opt.zero, opt.bgzf, opt.qv) if opt.emit_gpu else 0
        self.timers.add(run=t2 - t1, snapshot=time.perf_counter() - t2, **dev)
        with self.timers("wait_out"):
            self.to_fetch[w].put(b)
        return True

    def device_stage(self, w):                      # one per GPU: c3_batch_run sizes its stages on the host, so it blocks
        opt, tm = self.opt, self.timers
        cur = nxt = None                            # the batches this stage holds: to_fetch.put hands one on, the rest is released below
        try:
            with tm("setup"):
                h = self.handles[w] = _lib.Handle(device=opt.devices[w], mdistcutoff=opt.mdistcutoff, zero=1 if opt.zero else 0, zero_max_cells=opt.zero_max_cells)
                h.set_splints(self.splints)
            tm.put("at_setup_done")
            # software pipeline on one handle: while batch i runs, batch i+1 (if a reader already has it) is copied
            # and 2-bit packed on the handle's second stream (c3_batch_stage); c3_batch_commit makes it resident once
            # the results of batch i have been fetched
            cur = self.take(w)
            tm.put("at_first_batch")
            if cur is not None and not self.errors:
                with tm("upload"):
                    h.upload_host(cur.hb, cur.st, np.maximum(cur.sid, 0))
            done = cur is None
            while not done and not self.errors:
                if self.fused:
                    self.find_splints(h, cur)
                nxt, staged = None, False
                try:
                    nxt = self.take(w, False)
                    if nxt is not None:
                        with tm("upload"):
                            h.stage_host(nxt.hb, nxt.st, np.maximum(nxt.sid, 0))
                        staged = True
                    else:
                        done = True
                except queue.Empty:
                    pass
                if not self.run_batch(w, h, cur):
                    break
                cur = None
                if done:
                    break
                if nxt is None:                                   # no reader was ahead: wait for one now
                    nxt = self.take(w)
                    if nxt is None:
                        break
                with tm("upload"):
                    h.commit() if staged else h.upload_host(nxt.hb, nxt.st, np.maximum(nxt.sid, 0))
                cur, nxt = nxt, None
            tm.put("at_last_run_done")
            with tm("close"):
                self.fetched[w].wait()              # the last snapshot has been copied out
                h.close()
        except Exception as e:                      # noqa: BLE001
            self.errors.append(e)
        self.release(cur, nxt)
        with contextlib.suppress(Exception):
            while self.live[w]:                     # keep draining so no reader blocks on a full queue
                self.release(self.take(w))
        self.to_fetch[w].put(None)

    def fetch_stage(self, w):                       # c3_batch_results_fetch of batch i beside the kernels of batch i+1
        opt = self.opt
        while (b := self.to_fetch[w].get()) is not None:
            h = self.handles[w]
            b.rb = self.free_results.get()
            b.eb = self.free_emit.get() if opt.emit_gpu else None
            t0 = time.perf_counter()
            try:
                if opt.emit_gpu:                    # the records alone (the prefix copy is small), then the finished streams
                    b.res, b.buf, b.coff = h.results_fetch(b.rb, b.shape, with_cons=False)
                    b.eb, b.so = h.emit_fetch(b.eb, b.n_streams)
                    et = h.emit_timing()
                    self.timers.add(emit_bytes=et["out_bytes"], emit_records=et["n_records"],
                                    **{"emit_" + k: et["ms_" + k] * 1e-3 for k in ("len", "scan", "write", "bgzf", "call")})
                elif opt.qv:
                    b.res, b.buf, b.coff, b.qv = h.results_fetch_qv(b.rb, b.shape)
                else:
                    b.res, b.buf, b.coff = h.results_fetch(b.rb, b.shape)
            except Exception as e:                  # noqa: BLE001
                self.errors.append(e)
                self.fetched[w].set()
                self.release(b)                     # the buffers of a batch that is lost go back to their owners
                continue
            self.fetched[w].set()
            self.timers.add(fetch=time.perf_counter() - t0)
            self.to_write[w].put(b)
        self.to_write[w].put(None)

    def writer_stage(self, w):                      # c3_write_group releases the GIL: overlaps parsing and the GPUs
        opt, tree = self.opt, self.tree
        z = None                                    # --bgzf: this writer's c3_bgzf, on its worker's device
        while (b := self.to_write[w].get()) is not None:
            try:
                with self.timers("write"):
                    if self.errors:
                        pass
                    elif opt.emit_gpu:              # finished bytes (text, or BGZF members with --bgzf): appended, nothing formatted here
                        _lib.append_streams(tree.emit_paths, b.eb.ptr, b.so)
                    elif opt.bgzf:
                        if z is None:
                            z = _lib.Bgzf(opt.devices[w])
                        _lib.write_group_bgzf(z, b.hb, b.res, b.buf, b.coff, b.sid, tree.cons_w, tree.sub_w, opt.zero)
                        if opt.qv:
                            _lib.write_consensus_fastq_bgzf(z, b.hb, b.res, b.buf, b.coff, b.qv, b.sid, tree.fq_w, opt.zero)
                    else:
                        _lib.write_group(b.hb, b.res, b.buf, b.coff, b.sid, tree.cons_w, tree.sub_w, opt.zero)
                        if opt.qv:
                            _lib.write_consensus_fastq(b.hb, b.res, b.buf, b.coff, b.qv, b.sid, tree.fq_w, opt.zero)
            except Exception as e:                  # noqa: BLE001
                self.errors.append(e)
            self.release(b)
        if z is not None:
            z.close()

    def run(self):
        """starts the stages and returns when ALL of them have ended, after an error as well: the readers stop at `while not
        errors` and always post their end marker, and the device stage's drain keeps their queues moving"""
        def threads(stage, n):
            return [threading.Thread(target=stage, args=(i,), name="c3-%s-%d" % (stage.__name__, i), daemon=True) for i in range(n)]
        n_work, rthreads = self.opt.n_work, threads(self.reader_stage, len(self.readers))
        others = threads(self.writer_stage, n_work) + threads(self.fetch_stage, n_work) + threads(self.device_stage, n_work)
        self.timers.start = time.perf_counter()
        for th in rthreads + others:
            th.start()
        for th in others:
            th.join()
        self.timers.put("at_workers_done")
        for th in rthreads:
            th.join()


def run(args, splint_dict, assigner, adapter_set=None, n_dev=1, stats=None, finder_psl=None, keep_pinned=False):
    """the second pass of C3POa.py:236-271.  assigner: _lib.Assigner (native PSL table) or an adapter_dict.
    assigner=None is the fused mode: no PSL exists yet, so every batch is first scored against all splints on both
    strands (c3_scan_splints), assigned on the device (c3_batch_assign) and its PSL rows appended to finder_psl -- one pass
    over the reads instead of finder pass + counting pass + consensus pass.  returns the number of reads sent to the GPUs."""
    splint_names = sorted(splint_dict)
    if isinstance(assigner, dict):
        assigner = DictAssigner(assigner, splint_names)
    fused = assigner is None
    opt = Options.read(args, n_dev)
    if opt.bam and not opt.emit_gpu:
        raise ValueError("--bam needs --emit gpu: BAM records are made on the GPU only")
    tree = OutputTree(opt.out_path, splint_names, opt.bgzf, opt.compress, opt.qv, finder_psl if fused else None, bam=opt.bam)
    used = set(adapter_set or ())                   # cat_files runs per adapter_set entry (C3POa.py:259)
    if isinstance(assigner, DictAssigner):
        used |= set(v[0] for v in assigner.d.values())
    tree.prepare(used)
    readers, n_ranges = open_readers(opt)
    _lib.load().c3_writer_reset()
    timers = Timers(n_ranges, opt.emit_gpu)
    pipe = Pipeline(opt, tree, readers, [splint_dict[n][0] for n in splint_names], assigner, timers)
    kept = []
    try:
        pipe.run()
        if pipe.errors:
            raise pipe.errors[0]                    # the first error wins; it leaves through the finally below
        timers.put(inflate_wait=sum(r.inflate_wait() for r in readers))         # BGZF input: the parser waiting for inflated bytes
        if readers[0].parse_device:                 # --parse gpu: stretches parsed on the device / host, records from the device
            timers.put(**dict(zip(("parse_stretches_device", "parse_stretches_host", "parse_records_device"), (sum(x) for x in zip(*(r.parse_stats() for r in readers))))))
        if opt.gunzip_gpu:                          # --gunzip gpu: what went through the serial fallback instead of the kernels
            gz = readers[0].gunzip_stats()
            if gz["fallback_bytes"]:
                print("C3POa: --gunzip gpu: %d bytes of the input (%d stretches, %d block starts found) were inflated serially on the host: "
                      "streams of fixed or stored blocks, or of very many members, are read faster with --gunzip host"
                      % (gz["fallback_bytes"], gz["stretches"], gz["candidates"]), file=sys.stderr)
        if keep_pinned:                             # one-shot process (the CLI): process teardown releases the page-locked buffers
            kept = readers + pipe.emit_bufs         # ... and the page-locked arenas of --emit gpu likewise
            _KEPT.extend(kept)
    finally:
        for x in (() if kept else readers + pipe.emit_bufs + pipe.result_bufs):
            x.close()
    timers.put("at_readers_closed")
    tree.finish(pipe.seen if fused else None)
    if fused:
        timers.put(adapter_set=sorted(pipe.seen))
    t = timers.t
    if stats is not None:
        stats.update(t)
    if os.environ.get("C3_STREAM_STATS"):
        print("stream: " + " ".join("%s=%.3f" % (k, v) if isinstance(v, float) else "%s=%s" % (k, v) for k, v in t.items()), file=sys.stderr)
    return t["reads"]
