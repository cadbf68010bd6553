#!/usr/bin/env python3
"""C3POa_demux.py -- CLI of the sample demultiplexer (paper/Demultiplex_R2C2_reads.py of the reference).

Same flags and output file:
    python3 C3POa_demux.py -i R2C2_Consensus.fasta -o out -n Nextera_Indexes.fasta -t TSO_Indexes.fasta
Writes <out>/Indexed_reads.fasta: every read longer than 300 bases, renamed name|<Nextera>_<TSO> (an empty field where a
set makes no call).  -n is the Nextera index file here, not a GPU count; the index search runs on GPU 0.
--emit gpu reads the input as raw bytes and parses, searches and formats it on the GPU (c3_demux_emit): the same file, without
a Python loop over the reads; inputs only the host path reads like the reference (non-ASCII bytes, repeated headers, a
headless file) fall back to it with a note on stderr.
"""
import argparse
import json
import os
import sys

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
    p.add_argument("--demux-chunk", type=int, default=None, help=argparse.SUPPRESS)       # bytes of input per device call
    p.add_argument("--emit-stats", action="store_true", help=argparse.SUPPRESS)           # one JSON line on stderr
    return p.parse_args(argv)


def main(args):
    from c3poa_amd import demux
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


if __name__ == "__main__":
    sys.exit(main(parse_args()))
