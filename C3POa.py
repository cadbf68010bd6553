#!/usr/bin/env python3
"""C3POa.py -- drop-in CLI of the MI355X-native R2C2 consensus caller.

Same flags, inputs and output tree as rvolden/C3POa v2.2.3 (/root/reference/C3POa.py:26-63, 175-272):
    python3 C3POa.py -r reads.fastq|reads.bam -s splint.fasta -o out -c config -l 1000 -d 500 -n N -g 1000 [-z] [-b] [-co]
writes <out>/c3poa.log, <out>/tmp/splint_to_read_alignments.psl (reused when present),
<out>/<splint>/R2C2_Consensus.fasta[.gz] and <out>/<splint>/R2C2_Subreads.fastq[.gz].

Differences, all deliberate: the per-read hot path runs on the GPU(s) through
libc3poa_hip.so instead of conk/pyabpoa/mappy/racon; -n selects how many GPUs share the groups;
the last, short group is flushed (the reference never dispatches it);
racon/blat config entries are accepted, racon is never executed.
"""
import argparse
import os
import sys

PATH = os.path.dirname(os.path.realpath(__file__))
sys.path.insert(0, PATH)

from c3poa_amd import VERSION  # noqa: E402
from c3poa_amd.seqio import fastx_read, revcomp  # noqa: E402


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Makes consensus sequences from R2C2 reads.", add_help=True, prefix_chars="-")
    parser.add_argument("--reads", "-r", type=str, action="store", help="File that contains the long R2C2 reads: FASTQ (plain, gzip or BGZF) or an unaligned BAM "
                             "(.bam, as basecallers write it; an aligned BAM is refused: convert it with samtools fastq).")
    parser.add_argument("--splint_file", "-s", type=str, action="store", help="Path to the splint FASTA file.")
    parser.add_argument("--out_path", "-o", type=str, action="store", default=os.getcwd(),
                        help="Directory where all the files will end up. Defaults to your current directory.")
    parser.add_argument("--config", "-c", type=str, action="store", default="",
                        help="Config file with paths to racon and blat (tab separated).")
    parser.add_argument("--lencutoff", "-l", type=int, action="store", default=1000,
                        help="Sets the length cutoff for your raw sequences. Defaults to 1000.")
    parser.add_argument("--mdistcutoff", "-d", type=int, action="store", default=500,
                        help="Sets the median distance cutoff for consensus sequences. Defaults to 500.")
    parser.add_argument("--zero", "-z", action="store_false", default=True,
                        help="Use to exclude zero repeat reads. Defaults to True (includes zero repeats).")
    parser.add_argument("--zero-max-cells", dest="zero_max_cells", type=int, default=16777216,
                        help="Largest product of the two dangling piece lengths for which the zero-repeat rescue is "
                             "tried (1..2147483647). The reference has no cap; raise this for long-insert libraries, "
                             "whose zero-repeat reads have pieces of 4-8 kb. Defaults to 16777216.")
    parser.add_argument("--numThreads", "-n", type=int, default=1, help="Number of GPUs (workers) to use. Defaults to 1.")
    parser.add_argument("--groupSize", "-g", type=int, default=1000,
                        help="Number of reads processed by each worker in each iteration. Defaults to 1000.")
    parser.add_argument("--splint-finder", dest="splint_finder", choices=["gpu", "blat"], default="gpu",
                        help="How reads are assigned to splints when the PSL does not exist yet: the GPU finder "
                             "(default) or the blat binary of the config file, as upstream (FASTQ input only: a .bam is refused).")
    parser.add_argument("--blatThreads", "-b", action="store_true", default=False, help="Accepted for compatibility.")
    parser.add_argument("--compress_output", "-co", action="store_true", default=False,
                        help="Use to compress (gzip) both the consensus fasta and subread fastq output files.")
    parser.add_argument("--bgzf", action="store_true", default=False,
                        help="Compress the outputs to BGZF on the GPU while the run goes (implies -co: the same .gz file "
                             "names, readable by gzip, without an uncompressed file or a pass after the run). Off by default.")
    parser.add_argument("--inflate", choices=["host", "gpu"], default="host",
                        help="Where a BGZF .gz or a .bam input is inflated: zlib threads on the host (default), or the GPU (the "
                             "inflater threads' cores go back to the parser and the writers). Any other gzip file is read "
                             "as before.")
    parser.add_argument("--gunzip", choices=["host", "gpu"], default="host",
                        help="Where a plain gzip input (one deflate stream, as MinKNOW, guppy and gzip write it) is inflated: one zlib "
                             "stream on the host (default), or in parallel on the GPU (needs --inflate gpu). BGZF, .bam and plain text are "
                             "read as without it.")
    parser.add_argument("--parse", choices=["host", "gpu"], default="host",
                        help="Where the records of a BGZF .gz or a .bam input are found: the reader's parser thread on the host "
                             "(default), or the GPU, where --inflate gpu has left the text (needs --inflate gpu; strict "
                             "four-line FASTQ is parsed there, anything else by the host parser as before; the records of "
                             "an unaligned BAM are decoded there, and a record it cannot take is an error on either path).")
    parser.add_argument("--consensus-fastq", dest="consensus_fastq", action="store_true", default=False,
                        help="Also write <splint>/R2C2_Consensus.fastq: every consensus with per-base support QVs computed on "
                             "the GPU (not calibrated error probabilities; see DESIGN.md). Off by default.")
    parser.add_argument("--emit", choices=["host", "gpu"], default="host",
                        help="Where the consensus and subread records are formatted: the writer threads on the host "
                             "(default), or the GPU, while the batch is still resident (with --bgzf they are compressed there "
                             "as well). The files are the same byte for byte; measured at 1 M reads the run is slower "
                             "without --bgzf and faster with it (DESIGN.md 5.8).")
    parser.add_argument("--bam", action="store_true", default=False,
                        help="Write <splint>/R2C2_Consensus.bam and R2C2_Subreads.bam, unaligned BAM made and compressed on the GPU, "
                             "instead of the FASTA and FASTQ files (needs --emit gpu). A consensus record carries np, rl and aq "
                             "tags and, with --consensus-fastq, its QVs as qualities; --bgzf and -co change nothing for .bam "
                             "files. Read names of more than 219 bytes are refused. No index, no @RG (DESIGN.md 5.15).")
    parser.add_argument("--version", "-v", action="version", version=VERSION, help="Prints the C3POa version.")
    if argv is None and len(sys.argv) == 1:
        parser.print_help()
        sys.exit(0)
    args = parser.parse_args(argv)
    if args.bgzf:
        args.compress_output = True
    if args.gunzip == "gpu" and args.inflate != "gpu":
        parser.error("--gunzip gpu needs --inflate gpu: it says how a plain gzip input is inflated on the GPU")
    if args.bam and args.emit != "gpu":
        parser.error("--bam needs --emit gpu: BAM records are packed on the GPU while the batch is resident")
    if args.parse == "gpu" and args.inflate != "gpu":
        parser.error("--parse gpu needs --inflate gpu: records are parsed on the GPU only where the text was inflated there")
    return args


def configReader(path, configIn):
    """C3POa.py:65-84: tab separated name<TAB>path, '#' comments, missing keys fall back to PATH"""
    progs = {}
    with open(configIn) as f:
        for line in f:
            if line.startswith("#") or not line.rstrip().split():
                continue
            line = line.rstrip().split("\t")
            progs[line[0]] = line[1]
    for missing in set(["racon", "blat"]) - set(progs):
        progs[missing] = missing
        sys.stderr.write("Using " + str(missing) + " from your path, not the config file.\n")
    return progs


_WARMERS = []            # context-warming threads of main(); joined before a one-shot process leaves


def early_warm(n_threads):
    """The HIP context of every GPU in use takes 1.1-1.3 s to create and everything else waits for it: start it on threads of
    their own BEFORE numpy and the package are imported (0.3-0.5 s), with nothing but ctypes -- the library is loaded here and
    found loaded by c3poa_amd._lib later.  Returns silently when there is no library or no GPU (main() reports that)."""
    import ctypes
    import threading
    lib_path = os.environ.get("C3POA_LIB", os.path.join(PATH, "c3poa_amd", "lib", "libc3poa_hip.so"))
    try:
        lib = ctypes.CDLL(lib_path)
        lib.c3_warm_device.argtypes = [ctypes.c_int]
    except (OSError, AttributeError):
        return
    if os.environ.get("C3_DEVICE_MAP"):
        devs = sorted(set(int(x) for x in os.environ["C3_DEVICE_MAP"].split(",")))
    else:
        devs = list(range(max(1, n_threads)))                            # (an ordinal beyond the visible GPUs returns an error code at once)
    for dev in devs:
        th = threading.Thread(target=lib.c3_warm_device, args=(dev,), daemon=True)
        th.start()
        _WARMERS.append(th)


def main(args, one_shot=False):
    """one_shot: the process ends right after this call (the command line): the page-locked reader buffers are then left to
    process teardown instead of being unpinned one by one (1.2 s per 5 GB)"""
    if not args.out_path.endswith("/"):
        args.out_path += "/"
    os.makedirs(args.out_path, exist_ok=True)
    log_file = open(args.out_path + "c3poa.log", "w+")
    if args.config:
        progs = configReader(args.out_path, args.config)
        racon, blat = progs["racon"], progs["blat"]
    else:
        racon, blat = "racon", "blat"
    tmp_dir = args.out_path + "tmp/"
    os.makedirs(tmp_dir, exist_ok=True)

    from c3poa_amd import stream, _lib
    from c3poa_amd.preprocess import ensure_psl
    import time
    t_main = [time.perf_counter()]
    splint_dict = {}
    for splint in fastx_read(args.splint_file):
        splint_dict[splint[0]] = [splint[1], revcomp(splint[1])]
    n_dev = max(1, min(max(1, args.numThreads), _lib.device_count()))        # -n = GPUs that share the groups
    if os.environ.get("C3_DEVICE_MAP"):                                      # test hook: worker w -> device map[w] (e.g. "0,0": the -n 2
        n_dev = max(1, min(max(1, args.numThreads), len(os.environ["C3_DEVICE_MAP"].split(","))))      # plumbing on a one-GPU box)
    # the HIP context of every device in use is created NOW, on threads of its own, beside the PSL load / the first parse
    # (1.2-1.9 s each; the workers' handles then find their context ready)
    import threading
    dmap_ = [int(x) for x in os.environ["C3_DEVICE_MAP"].split(",")] if os.environ.get("C3_DEVICE_MAP") else list(range(n_dev))

    if not _WARMERS:                                                         # (the command line has started them before its imports: early_warm)
        warmers = [threading.Thread(target=_lib.warm_device, args=(dev,), daemon=True) for dev in sorted(set(dmap_[:n_dev]))]
        for th in warmers:                                                   # (context only: a failure is reported by the worker's own c3_create)
            th.start()
        _WARMERS.extend(warmers)
    align_psl = tmp_dir + "splint_to_read_alignments.psl"
    have_psl = os.path.exists(align_psl) and os.stat(align_psl).st_size > 0
    if not have_psl and getattr(args, "splint_finder", "gpu") == "gpu":
        # no PSL yet: ONE pass over the reads -- every batch is scored against all splints on both strands on the GPU,
        # assigned, processed; the PSL (written on the way) makes a rerun take the route below
        print("Assigning splints to reads on the GPU", file=sys.stderr)
        st = {}
        stream.run(args, splint_dict, None, None, n_dev, stats=st, finder_psl=align_psl, keep_pinned=one_shot)
        total_reads, short_reads, no_splint = st["reads"], st["short"], st["reads"] - st["assigned"]
        t_main += [time.perf_counter()] * 3
    else:
        # splint / strand per read from the PSL (bin/preprocess.py:12-45).  The PSL is reused when it exists (or written by
        # blat); it is held in a native name -> (splint, strand) table.  The reference's first pass over the reads
        # (C3POa.py:200-207) only counts them for the log: those counts fall out of the one streaming pass below.
        assigner = _lib.Assigner(ensure_psl(blat, args, tmp_dir), sorted(splint_dict))
        t_main.append(time.perf_counter())
        adapter_set, _rows = assigner.seen()
        for adapter in adapter_set:
            os.makedirs(args.out_path + adapter, exist_ok=True)
        t_main.append(time.perf_counter())
        # streaming pipeline: native readers -> GPU batches -> native writers (c3poa_amd/stream.py); the tail group is
        # processed too (deliberate fix of SURVEY.md App. A.12)
        st = {}
        stream.run(args, splint_dict, assigner, adapter_set, n_dev, stats=st, keep_pinned=one_shot)
        total_reads, short_reads, no_splint = st["reads"], st["short"], st["reads"] - st["assigned"]
        if not one_shot:
            assigner.close()
        t_main.append(time.perf_counter())

    all_reads = total_reads + short_reads
    print("C3POa version:", VERSION, file=log_file)
    print("Total reads:", all_reads, file=log_file)
    if all_reads:
        print("No splint reads:", no_splint, "({:.2f}%)".format((no_splint / all_reads) * 100), file=log_file)
        print("Under len cutoff:", short_reads, "({:.2f}%)".format((short_reads / all_reads) * 100), file=log_file)
        print("Total thrown away reads:", short_reads + no_splint,
              "({:.2f}%)".format(((short_reads + no_splint) / all_reads) * 100), file=log_file)
    print("Reads after preprocessing:", all_reads - (short_reads + no_splint), file=log_file)
    log_file.close()
    if os.environ.get("C3_STREAM_STATS"):
        print("main: psl=%.3f count=%.3f consensus=%.3f" % tuple(b - a for a, b in zip(t_main, t_main[1:4])), file=sys.stderr)


if __name__ == "__main__":
    args = parse_args()
    if not args.reads or not args.splint_file:
        print("Reads (--reads/-r) and splint (--splint_file/-s) are required", file=sys.stderr)
        sys.exit(1)
    if not os.environ.get("C3_NO_EARLY_WARM"):          # (A/B hook of tools/cli_throughput.py)
        early_warm(args.numThreads)
    main(args, one_shot=True)
    for th_ in _WARMERS:                          # never leave while a thread is still inside HIP initialisation
        th_.join()
    # every output file has been written and closed; skip the interpreter's and the HIP runtime's teardown (unpinning the reader
    # buffers, freeing the device scratch: ~1.5 s that produce nothing)
    sys.stdout.flush(); sys.stderr.flush()
    os._exit(0)
