// c3_reader_bgzf.h -- the BGZF input stream of the reader (c3_reader.cpp): the file taken apart into stretches of members that
// are inflated by zlib threads, inflated by k_inflate, or inflated and parsed on the device (c3_stream.hip).  (c3_bgzf.h is the
// host compressor.)
#pragma once
#include <atomic>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

#include "../../include/c3poa.h"
#include "c3_checks.h"

// BGZF input (bgzip / htslib): a gzip file made of independent members of <= 64 KiB whose header carries the member's size
// (extra subfield 'B','C'), so the members of a stretch of the file can be located WITHOUT inflating them and inflated by several
// threads at once -- a plain gzip stream is one zlib state and inflates at ~275 MB/s whatever the machine (27 k reads/s:
// profiles/r04_host_ceiling_gz.txt).  Plain gzip stays on gzread.
// a stretch that stays on the device (c3_reader_parse_on_device): c3_stream.hip inflates it behind the record the previous
// stretch's end cut, parses it with k_fastq and keeps the finished records until the slot is loaded again
// (c3_fq_stretch, c3_bgzf_stretch_*: c3_checks.h)

struct BgzfStretch {
  std::vector<unsigned char> comp;          // compressed members of the stretch, back to back
  std::vector<size_t> coff, csz, doff;      // per member: offset / size in comp, offset of its data in dec
  std::vector<char> dec;                    // inflated stretch
  size_t dend = 0;
  bool on_dev = false;                      // parsed on the device: fq describes its records, next_rec is the first not yet in a group
  c3_fq_stretch fq{};
  int64_t next_rec = 0;
  int64_t base_off = 0;                     // BAM: inflated file offset of the stretch's first byte (error texts)
};
struct Bgzf {
  FILE* fp = nullptr;
  // c3_reader_gunzip_on_device: not BGZF at all but a plain gzip file -- a stretch is what the gzip stream inflates next on dev
  // (k_gunzip), brought to dec or left on the device for the parser; everything else here stays as it is
  c3_gunzip_stream* gs = nullptr;
  int threads = 1;
  BgzfStretch st[2];                        // the stretch being parsed and the one being read + inflated beside it
  int cur = 0;
  size_t dpos = 0;                          // unread part of st[cur].dec starts here
  std::thread pre; bool pre_on = false, pre_ok = false;
  std::atomic<bool> eof{false}, bad{false};  // (written by the prefetch thread, read by the parser)
  c3_bgzf* dev = nullptr;                   // c3_reader_open_inflate: stretches are inflated by k_inflate, not by zlib threads
  std::string why;                          // the device call's error text (written before bad is set)
  double wait_s = 0;                        // the parser waiting for a stretch (c3_reader_inflate_wait)
  size_t stretch_members = 4096;            // members per device stretch (C3_INFLATE_STRETCH_MEMBERS)
  // c3_reader_parse_on_device: parse_req = asked for; parse_on = stretches are still loaded for the device parser (cleared at
  // the first departure, before the next load starts); dev_active = the reader thread still has device records to hand out
  bool parse_req = false, parse_on = false, dev_active = false;
  int64_t carry_from = 0, carry_len = 0;    // the next load starts with these bytes of the current stretch's text
  std::atomic<int64_t> n_dev{0}, n_host{0}, rec_dev{0};
  // c3_reader_stage_on_device: while dev_active, groups stay on the device (one device set per host set, held by dev)
  bool stage_on = false;
  int64_t grp_dev = 0, grp_host = 0, host_bytes = 0;
  // a .bam file: the device stretches go through k_bam; at_start until a stretch has consumed the file header; dev_base =
  // inflated bytes consumed by the stretches in front of the current one
  bool bam = false, bam_at_start = true;
  int64_t dev_base = 0;
};
// header of a BGZF member at p (n bytes available): total member size, or 0 when it is not one
size_t bgzf_member_size(const unsigned char* p, size_t n);
// bytes of the inflated file, in order: up to `room` of them; 0 at the end of the file, -1 when a member is damaged (b->bad)
long bgzf_read(Bgzf* b, char* dst, size_t room);
// device parse: the next stretch becomes the current one.  false: nothing more was loaded (end of file, or b->bad)
bool dev_advance(Bgzf* b);
