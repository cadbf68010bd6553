#!/usr/bin/env python3
"""C3POa_postprocessing.py -- drop-in CLI of the post-processing step (trim / re-orient / demultiplex consensus reads).

Same flags, inputs and output files as rvolden/C3POa v2.2.3 (/root/reference/C3POa_postprocessing.py:17-62, 400-434):
    python3 C3POa_postprocessing.py -i R2C2_Consensus.fasta -a adapters.fasta -o out [-x indexes.fasta] [-u] [-t] [-b]
                                    [-n N] [-g 1000] [-bt] [-co] [-c config] [--emit gpu [--keep-quals] [--bgzf] [--parse gpu [--inflate gpu]]]
The adapter-to-read alignment that upstream delegates to blat runs on the GPU (c3_scan_adapters); the PSL file
<out>/adapter_to_consensus_alignment.psl is written and reused exactly as upstream reuses it.
"""
import argparse
import os
import sys

PATH = os.path.dirname(os.path.realpath(__file__))
sys.path.insert(0, PATH)

from c3poa_amd import VERSION  # noqa: E402


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Reorients/demuxes/trims consensus reads.", add_help=True, prefix_chars="-")
    p.add_argument("--input_fasta_file", "-i", type=str, action="store", help="Fasta file with consensus called R2C2 reads")
    p.add_argument("--output_path", "-o", type=str, action="store", default=os.getcwd(),
                   help="Directory where all the files will end up. Defaults to your current directory.")
    p.add_argument("--adapter_file", "-a", type=str, action="store", help="Fasta file with adapter (3 and 5 prime) sequences")
    p.add_argument("--index_file", "-x", type=str, action="store", help="Fasta file with oligo dT indexes")
    p.add_argument("--config", "-c", type=str, action="store", default="", help="Accepted for compatibility (program paths).")
    p.add_argument("--undirectional", "-u", action="store_true",
                   help="cDNA molecules are undirectional: one sequence named 'Adapter' in the adapter file "
                        "(default: '3Prime_adapter' and '5Prime_adapter').")
    p.add_argument("--trim", "-t", action="store_true", help="Trim the adapters off the ends of the sequences.")
    p.add_argument("--barcoded", "-b", action="store_true", default=False,
                   help="10x reads: also writes a file with the 10x barcode sequences.")
    p.add_argument("--threads", "-n", type=int, default=1, help="Accepted for compatibility; > 1 selects upstream's multi-process output conventions.")
    p.add_argument("--groupSize", "-g", type=int, default=1000, help="Accepted for compatibility.")
    p.add_argument("--blatThreads", "-bt", action="store_true", default=False, help="Accepted for compatibility.")
    p.add_argument("--compress_output", "-co", action="store_true", default=False, help="gzip the output files (with -n > 1, as upstream).")
    p.add_argument("--adapter-finder", dest="adapter_finder", choices=["gpu"], default="gpu", help="How adapters are located (GPU local alignment).")
    p.add_argument("--emit", choices=["host", "gpu"], default="host",
                   help="gpu: classify, trim, orient, demultiplex and format the records on the GPU (k_post); host (default): as before.")
    p.add_argument("--keep-quals", dest="keep_quals", action="store_true", default=False,
                   help="Carry the qualities of a FASTQ input through: the three read files become .fastq (needs --emit gpu).")
    p.add_argument("--bgzf", action="store_true", default=False,
                   help="Write the read files (three per destination, and the 10x file) as BGZF <name>.gz, compressed on the GPU "
                        "(k_bgzf) as they are written; the TSV and the PSL stay plain (needs --emit gpu; not with -co).")
    p.add_argument("--parse", choices=["host", "gpu"], default="host",
                   help="gpu: the input goes to the GPU as text, piece by piece, and is parsed there (k_fastx); only finished file "
                        "bytes come back (needs --emit gpu).  host (default): the reader parses, as before.")
    p.add_argument("--inflate", choices=["host", "gpu"], default="host",
                   help="gpu: a BGZF input is inflated on the GPU as well (k_inflate; needs --parse gpu).")
    p.add_argument("--post-chunk", dest="post_chunk", type=int, default=64 << 20, help=argparse.SUPPRESS)
    p.add_argument("--emit-stats", dest="emit_stats", action="store_true", default=False, help=argparse.SUPPRESS)
    p.add_argument("--post-batch", dest="post_batch", type=int, default=200000, help=argparse.SUPPRESS)
    p.add_argument("--version", "-v", action="version", version=VERSION, help="Prints the C3POa version.")
    if argv is None and len(sys.argv) == 1:
        p.print_help()
        sys.exit(0)
    args = p.parse_args(argv)
    if args.keep_quals and args.emit != "gpu":
        p.error("--keep-quals needs --emit gpu")
    if args.bgzf and args.emit != "gpu":
        p.error("--bgzf needs --emit gpu")
    if args.parse == "gpu" and args.emit != "gpu":
        p.error("--parse gpu needs --emit gpu")
    if args.inflate == "gpu" and args.parse != "gpu":
        p.error("--inflate gpu needs --parse gpu")
    if args.post_chunk < 1:
        p.error("--post-chunk must be at least 1")
    if args.bgzf and args.compress_output:
        p.error("-co and --bgzf both compress the output: give one of them")
    return args


def main(args):
    from c3poa_amd import postprocess
    return postprocess.run(args)


if __name__ == "__main__":
    args = parse_args()
    if not args.input_fasta_file or not args.adapter_file:
        print("Reads (--input_fasta_file/-i) and adapter (--adapter_file/-a) are required", file=sys.stderr)
        sys.exit(1)
    main(args)
