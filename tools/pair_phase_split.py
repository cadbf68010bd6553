#!/usr/bin/env python3
"""k_poa's wave time split by alignment (diagnostic build: make -C c3poa_amd/csrc prof):
   C3POA_LIB=c3poa_amd/lib/libc3poa_hip_prof.so python tools/pair_phase_split.py [n_reads] [cfg]
tools/phase_prof.py runs twice on the same batch: with C3_DEBUG_POA_PAIR=0, where k_poa aligns every subread itself (the parent's
path), and by default, where the reads k_poa_pair has taken skip poa_align at s == 1.  The phase counters of k_poa cover only
what k_poa runs, so their difference is what the s == 1 alignments of the taken reads cost inside k_poa (init + descriptors,
rows by kind, traceback), and the second run is what is left: s >= 2 plus the s == 1 alignments of declined reads.  n_pair of
the second run is the number of reads whose s == 1 alignment has every row at most 128 columns wide and Q1 <= 1792."""
import ast
import os
import subprocess
import sys

here = os.path.dirname(os.path.abspath(__file__))
args = sys.argv[1:] or ["32768", "cfg2"]


def run(extra):
    env = dict(os.environ, **extra)
    out = subprocess.run([sys.executable, os.path.join(here, "phase_prof.py")] + args, env=env, capture_output=True, text=True).stdout
    raw = [l for l in out.splitlines() if l.startswith("k_poa raw")]
    tim = [l for l in out.splitlines() if "ms_total" in l]
    if not raw or not tim:
        sys.exit("phase_prof.py gave no counters (is C3POA_LIB the diagnostic build?)\n" + out[-2000:])
    return [int(x) for x in raw[0].split()[2:]], ast.literal_eval(tim[0]), out


off, t_off, text_off = run({"C3_DEBUG_POA_PAIR": "0"})
on, t_on, text_on = run({})
print("# C3_DEBUG_POA_PAIR=0 (k_poa aligns every subread)")
print(text_off.strip())
print("# default (k_poa_pair ahead of k_poa)")
print(text_on.strip())
tot = float(sum(off[:8]) + off[9])
lo = lambda x: x & 0xffffffff          # noqa: E731
hi = lambda x: x >> 32                 # noqa: E731
print("# k_poa wave time with the kernel off = 100 %%; s == 1 of the reads taken = off - on; the rest = on")
for name, i in (("init + descriptors", 0), ("rows", 1), ("traceback", 2)):
    print("  %-20s all %5.1f%%   s == 1 (taken reads) %5.1f%%   s >= 2 and declined %5.1f%%" % (name, 100 * off[i] / tot, 100 * (off[i] - on[i]) / tot, 100 * on[i] / tot))
for name, i, cnt in (("fast rows", 8, lo), ("two-column rows", 15, hi), ("near rows", 10, None), ("general rows", 11, None)):
    n1 = (cnt(off[12]) - cnt(on[12])) if cnt else 0
    print("  %-20s cycles: all %5.1f%%   s == 1 %5.1f%%%s" % (name, 100 * off[i] / tot, 100 * (off[i] - on[i]) / tot,
                                                             "   (%d rows at %.0f cycles)" % (n1, (off[i] - on[i]) / max(n1, 1)) if cnt else ""))
share = sum(off[i] - on[i] for i in (0, 1, 2)) / tot
print("  s == 1 in the three phases: %.1f%% of k_poa's wave time; other phases moved by %.1f%%" % (100 * share, 100 * (sum(off[3:8]) + off[9] - sum(on[3:8]) - on[9]) / tot))
n2 = t_on["n_pair"] + t_on["n_pair_declined"]
print("  reads with >= 2 subreads %d: eligible and taken (n_pair) %d, declined %d" % (n2, t_on["n_pair"], t_on["n_pair_declined"]))
print("  ms_poa %.2f -> %.2f (diagnostic build), of which k_poa_pair %.2f" % (t_off["ms_poa"], t_on["ms_poa"], t_on["ms_poa_pair"]))
