"""Inputs of tools/reader_digest_host.sh, written into the directory given: the records of the BAM reader tests
(tests/test_bam_host.py: cfg2 reads with records of the edge corpus in between) as plain FASTQ and FASTA, plain gzip, BGZF FASTQ and
BAM at block sizes 4096 and 65280, a BAM with a departure, the multi-line / CRLF / no-final-newline / empty-record files of
tests/test_host_io.py, a truncated quality string and a BGZF file with one damaged member.  Prints the driver's arguments, one
per line (range3:PATH = three byte ranges that tile PATH).  Needs no GPU."""
import gzip
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bam_cases as B                      # noqa: E402
import test_bam_host as T                  # noqa: E402
import test_inflate_host as H              # noqa: E402


def main(out):
    recs = T.reader_records()[40:70]       # 10 cfg2 reads, the 20 edge records, 10 cfg2 reads
    fq = B.fastq_of(recs)
    fa = b"".join(b">%s\n%s\n" % (n, s.encode()) for n, s, _q in recs)
    bam = B.header(b"@HD\tVN:1.6\tSO:unsorted\n") + b"".join(T.record_with_tags(i, r) for i, r in enumerate(recs))
    good = [B.record(*r) for r in recs[:10]]
    departure = B.header() + b"".join(good[:7]) + B.record(b"rev", "ACGT", b"\x10" * 4, flag=0x10) + b"".join(good[7:])
    damaged = bytearray(H.bgzf_file(fq, block=4096))
    damaged[len(damaged) // 2] ^= 0x55
    files = [("reads.fastq", fq), ("reads.fasta", fa),
             ("edge.fa", b">s1 desc\tmore\nAC\nGT\n\n>s2\nTTT\r\n>s3\n>s4\tx\nGG"),
             ("edge.fq", b"@a\nACGT\nAC\n+a\n@III\nI@\n@b c\nGG\n+\n@@\n"),
             ("plain.fastq.gz", gzip.compress(fq, 6, mtime=0)),
             ("bgzf4096.fastq.gz", H.bgzf_file(fq, block=4096)), ("bgzf65280.fastq.gz", H.bgzf_file(fq, block=65280)),
             ("reads4096.bam", H.bgzf_file(bam, block=4096)), ("reads65280.bam", H.bgzf_file(bam, block=65280)),
             ("departure.bam", H.bgzf_file(departure, block=4096)),
             ("truncated_quality.fq", fq[:fq.index(b"\n+\n", len(fq) // 2) + 6] + b"\n" + fq[:400]),
             ("damaged.fastq.gz", bytes(damaged))]
    os.makedirs(out, exist_ok=True)
    for name, data in files:
        with open(os.path.join(out, name), "wb") as f:
            f.write(data)
        print(os.path.join(out, name))
    print("range3:" + os.path.join(out, "reads.fastq"))


if __name__ == "__main__":
    main(sys.argv[1])
