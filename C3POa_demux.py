#!/usr/bin/env python3
"""C3POa_demux.py -- CLI of the sample demultiplexer (paper/Demultiplex_R2C2_reads.py of the reference).

Same flags and output file:
    python3 C3POa_demux.py -i R2C2_Consensus.fasta -o out -n Nextera_Indexes.fasta -t TSO_Indexes.fasta
Writes <out>/Indexed_reads.fasta: every read longer than 300 bases, renamed name|<Nextera>_<TSO> (an empty field where a
set makes no call).  -n is the Nextera index file here, not a GPU count; the index search runs on GPU 0.
--emit gpu reads the input as raw bytes and parses, searches and formats it on the GPU (c3_demux_emit): the same file, without
a Python loop over the reads; inputs only the host path reads like the reference (non-ASCII bytes, repeated headers, a
headless file) fall back to it with a note on stderr.
--emit gpu --parse gpu takes what the tools before this one write: FASTA or FASTQ (by the first byte), plain, gzip or BGZF,
in pieces through the GPU (c3_demux_emit_text), and enables
    --inflate gpu   a BGZF input is inflated on the GPU (plain gzip, and BGZF without the flag, go through zlib on the host)
    --keep-quals    FASTQ input only: '@name|A_B / sequence / + / quality' records in <out>/Indexed_reads.fastq
    --split         one file per sample that received a read, <out>/samples/<Nextera>_<TSO>.fasta (.fastq), records in input
                    order, instead of Indexed_reads.*; an index name with '/' or NUL, or two pairs with one file name, is refused
    --bgzf          every output file as BGZF, <name>.gz, closed by one EOF member
    python3 C3POa_demux.py -i R2C2_Consensus.fastq.gz -o out -n Nextera.fasta -t TSO.fasta --emit gpu --parse gpu --inflate gpu --split --keep-quals --bgzf
Where the device path declines (a departure from the FASTA or the strict four-line FASTQ rule, a repeated name, an index name
holding '|' or a byte >= 0x80, more than 4096 sample streams, a refused call) the host path writes the same files, with a note
on stderr.
"""
import argparse
import json
import os
import sys
import zlib

PATH = os.path.dirname(os.path.realpath(__file__))
sys.path.insert(0, PATH)


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Renames consensus reads by the Nextera and TSO indexes they carry.")
    p.add_argument("-i", "--input_fasta_file", type=str, required=True, help="Fasta file with consensus called R2C2 reads")
    p.add_argument("-o", "--output_path", type=str, required=True, help="Directory for Indexed_reads.fasta (created if missing)")
    p.add_argument("-n", "--nextera_index_file", type=str, required=True, help="Fasta file with the Nextera indexes")
    p.add_argument("-t", "--tso_index_file", type=str, required=True, help="Fasta file with the TSO indexes")
    p.add_argument("--emit", choices=("host", "gpu"), default="host",
                   help="host: reads pass through Python (default); gpu: FASTA text is parsed, searched and formatted on the GPU")
    p.add_argument("--parse", choices=("host", "gpu"), default="host",
                   help="gpu (needs --emit gpu): FASTA, FASTQ, gzip or BGZF input in pieces through the GPU; enables --split, --keep-quals, --bgzf")
    p.add_argument("--inflate", choices=("host", "gpu"), default="host", help="gpu (needs --parse gpu): a BGZF input is inflated on the GPU")
    p.add_argument("--split", action="store_true", help="(needs --parse gpu) one file per sample, <out>/samples/<Nextera>_<TSO>.fasta, instead of Indexed_reads.fasta")
    p.add_argument("--keep-quals", dest="keep_quals", action="store_true",
                   help="(needs --parse gpu, FASTQ input) write FASTQ records with the input's qualities: Indexed_reads.fastq")
    p.add_argument("--bgzf", action="store_true", help="(needs --parse gpu) write every output file as BGZF, <name>.gz")
    p.add_argument("--demux-chunk", type=int, default=None, help=argparse.SUPPRESS)       # bytes of input per device call
    p.add_argument("--emit-stats", action="store_true", help=argparse.SUPPRESS)           # one JSON line on stderr
    # for the tests only, not for use: with host the host path of --parse gpu searches with c3_demux_host, so that the CPU tests can
    # run the CLI's host path without a device
    p.add_argument("--search", choices=("gpu", "host"), default="gpu", help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.parse == "gpu" and args.emit != "gpu":
        p.error("--parse gpu needs --emit gpu")
    for flag, on in (("--inflate gpu", args.inflate == "gpu"), ("--split", args.split), ("--keep-quals", args.keep_quals), ("--bgzf", args.bgzf),
                     ("--search host", args.search == "host")):
        if on and args.parse != "gpu":
            p.error("%s needs --parse gpu" % flag)
    return args


def main(args):
    from c3poa_amd import demux
    if args.parse == "gpu":
        return main_parse_gpu(args, demux)
    out_file = os.path.join(args.output_path, "Indexed_reads.fasta")
    if args.emit == "gpu":
        stats = {}
        try:
            done = demux.run_emit_gpu(args.input_fasta_file, args.output_path, args.nextera_index_file, args.tso_index_file,
                                      chunk=args.demux_chunk or demux.EMIT_CHUNK, stats=stats)
        except (demux.DemuxError, OSError, UnicodeDecodeError) as e:
            print("C3POa_demux: %s" % e, file=sys.stderr)
            return 1
        finally:
            if args.emit_stats:
                print(json.dumps(stats), file=sys.stderr)
        if done is not None:
            print("%d of %d reads written to %s" % (done[0], done[1], out_file))
            return 0
    try:
        reads = demux.read_fasta(args.input_fasta_file)
        indexed = demux.demultiplex(reads, args.nextera_index_file, args.tso_index_file)
    except (demux.DemuxError, OSError, UnicodeDecodeError) as e:
        print("C3POa_demux: %s" % e, file=sys.stderr)
        return 1
    os.makedirs(args.output_path, exist_ok=True)
    demux.write_fasta_file(args.output_path, indexed)
    print("%d of %d reads written to %s" % (len(indexed), len(reads), os.path.join(args.output_path, "Indexed_reads.fasta")))
    return 0


def main_parse_gpu(args, demux):
    """--emit gpu --parse gpu: the device path, then the host path for the same flags where the device path declines"""
    from c3poa_amd import _lib
    stats = {}
    kw = dict(split=args.split, keep_quals=args.keep_quals, bgzf=args.bgzf)
    try:
        try:
            done = demux.run_text_gpu(args.input_fasta_file, args.output_path, args.nextera_index_file, args.tso_index_file,
                                      inflate_gpu=args.inflate == "gpu", chunk=args.demux_chunk or demux.EMIT_CHUNK, stats=stats, **kw)
        finally:
            if args.emit_stats:
                print(json.dumps(stats), file=sys.stderr)
        if done is None:
            done = demux.run_text_host(args.input_fasta_file, args.output_path, args.nextera_index_file, args.tso_index_file,
                                       host_search=args.search == "host", stats=stats, **kw)
    except (demux.DemuxError, _lib.C3Error, OSError, UnicodeDecodeError, EOFError, zlib.error) as e:      # (zlib.error: a damaged deflate body)
        print("C3POa_demux: %s" % e, file=sys.stderr)
        return 1
    where = os.path.join(args.output_path, "samples") if args.split else os.path.join(args.output_path, demux._out_names(False, args.keep_quals, args.bgzf)[0])
    print("%d of %d reads written to %s" % (done[0], done[1], where))
    return 0


if __name__ == "__main__":
    sys.exit(main(parse_args()))
