// c3_io.cpp -- native host I/O either side of the hot path: streaming FASTA/FASTQ(.gz) reader that
// fills structure-of-arrays host batches in page-locked memory (so c3_batch_upload copies them by DMA), and the writer
// of the reference's two per-group output files.  Host code only: no kernels here, nothing here touches the oracle.
//
//   c3_reader_*      replaces mm.fastx_read(args.reads, read_comment=False)   (C3POa.py:201,239; kseq.h semantics)
//   c3_write_group   replaces the file side effects of analyze_reads + determine_consensus
//                    (C3POa.py:141-173, bin/determine_consensus.py:57-77,108-114)
#include <hip/hip_runtime.h>
#include <zlib.h>

#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <mutex>
#include <thread>
#include <sys/stat.h>
#include <unordered_map>
#include <vector>

#include "../../include/c3poa.h"
#include "c3_checks.h"
#include "c3_bam.h"
#include "c3_emit.h"

namespace {

// ---- growable host buffer, page-locked when a GPU runtime is present (plain malloc otherwise: pinning is a transfer
//      optimisation, not a compute path) -------------------------------------------------------------------------
struct HostBuf {
  char* p = nullptr; size_t cap = 0; bool pinned = false;
  ~HostBuf() { release(); }
  void release() {
    if (!p) return;
    if (pinned) (void)hipHostFree(p); else free(p);
    p = nullptr; cap = 0;
  }
  bool reserve(size_t need, size_t keep) {
    if (need <= cap) return true;
    size_t ncap = cap ? cap : (size_t)1 << 20;
    while (ncap < need) ncap += ncap / 2;
    char* q = nullptr; bool pin = false;
    static int can_pin = -1;
    if (can_pin < 0) { int n = 0; can_pin = (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? 1 : 0; (void)hipGetLastError(); }
    if (can_pin && hipHostMalloc((void**)&q, ncap, hipHostMallocDefault) == hipSuccess) pin = true;
    else { (void)hipGetLastError(); q = (char*)malloc(ncap); }
    if (getenv("C3_DEBUG")) fprintf(stderr, "[c3_io] host buffer %zu MiB %s\n", ncap >> 20, pin ? "page-locked" : "pageable");
    if (!q) return false;
    if (keep) memcpy(q, p, keep);
    release();
    p = q; cap = ncap; pinned = pin;
    return true;
  }
};

struct BatchSet {
  HostBuf names, seqs, quals;
  std::vector<int64_t> name_off, off;
  size_t n_names = 0, n_bases = 0;
  bool on_dev = false;                      // the group it holds is a device group: its bases lie in the reader's device set (c3_reader_stage_on_device)
};

}  // namespace

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

struct c3_reader {
  FILE* fp = nullptr; gzFile gz = nullptr; Bgzf* bz = nullptr;
  std::vector<char> buf; size_t beg = 0, end = 0; bool eof = false;
  std::vector<BatchSet> sets; int cur = -1;
  std::string err;
  bool have_line = false; const char* lp = nullptr; size_t ll = 0;   // one line of look-ahead
  int64_t n_records = 0, n_noqual = 0;
  bool names_only = false;
  bool started = false;         // c3_reader_next has been called
  bool range_lost = false;      // a byte range with bytes in it held no recognisable record start (e.g. multi-line FASTQ)
  size_t file_bytes = 0, hint_bases = 0;
  int64_t buf_off = 0;          // file offset of buf[0] (plain files)
  int64_t range_end = -1;       // byte range readers stop at the first record that starts at or after this offset
  bool bam = false;             // a .bam path: the inflated bytes are BAM records (c3_bam.h), not text
  bool bam_hdr = false;         // ... whose file header has been consumed
};

namespace {

// header of a BGZF member at p (n bytes available): total member size, or 0 when it is not one
size_t bgzf_member_size(const unsigned char* p, size_t n) {
  if (n < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
  const size_t xlen = (size_t)p[10] | ((size_t)p[11] << 8);
  if (12 + xlen > n) return 0;
  for (size_t q = 12; q + 4 <= 12 + xlen;) {
    const size_t slen = (size_t)p[q + 2] | ((size_t)p[q + 3] << 8);
    if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2 && q + 6 <= 12 + xlen) return ((size_t)p[q + 4] | ((size_t)p[q + 5] << 8)) + 1;
    q += 4 + slen;
  }
  return 0;
}

// inflate one member (raw deflate between the header and the 8-byte trailer), checking its CRC and size
bool bgzf_inflate(const unsigned char* m, size_t msz, char* out, size_t osz) {
  const size_t xlen = (size_t)m[10] | ((size_t)m[11] << 8);
  const size_t hdr = 12 + xlen;
  if (msz < hdr + 8) return false;
  z_stream z; memset(&z, 0, sizeof(z));
  if (inflateInit2(&z, -15) != Z_OK) return false;
  z.next_in = const_cast<unsigned char*>(m + hdr); z.avail_in = (unsigned)(msz - hdr - 8);
  z.next_out = (unsigned char*)out; z.avail_out = (unsigned)osz;
  const int rc = inflate(&z, Z_FINISH);
  const bool ok = rc == Z_STREAM_END && z.avail_out == 0;
  inflateEnd(&z);
  if (!ok) return false;
  const unsigned char* t = m + msz - 8;
  const unsigned long crc = (unsigned long)t[0] | ((unsigned long)t[1] << 8) | ((unsigned long)t[2] << 16) | ((unsigned long)t[3] << 24);
  return crc32(crc32(0L, Z_NULL, 0), (const unsigned char*)out, (unsigned)osz) == crc;
}

// next stretch of the file: up to `max_members` members read, located by their headers, inflated by b->threads threads
bool bgzf_next_stretch(Bgzf* bz, BgzfStretch* b, size_t max_members = 512) {
  if (bz->dev) max_members = bz->stretch_members;               // one k_inflate launch: a wave per member
  b->comp.clear(); b->coff.clear(); b->csz.clear(); b->doff.clear();
  b->dend = 0;
  size_t dtot = 0;
  unsigned char hd[18];
  while (b->coff.size() < max_members && !bz->eof) {
    const size_t got = fread(hd, 1, 18, bz->fp);
    if (got == 0) { bz->eof = true; break; }
    if (got < 18) { bz->bad = true; return false; }
    // the fixed part of the header holds the BC subfield when it comes first (every writer puts it there); otherwise read on
    size_t msz = bgzf_member_size(hd, 18);
    const size_t at = b->comp.size();
    if (!msz) {
      const size_t xlen = (size_t)hd[10] | ((size_t)hd[11] << 8);
      if (hd[0] != 0x1f || hd[1] != 0x8b || !(hd[3] & 4) || xlen > 65535) { bz->bad = true; return false; }
      b->comp.resize(at + 12 + xlen);
      memcpy(b->comp.data() + at, hd, 18);
      if (12 + xlen > 18 && fread(b->comp.data() + at + 18, 1, 12 + xlen - 18, bz->fp) != 12 + xlen - 18) { bz->bad = true; return false; }
      msz = bgzf_member_size(b->comp.data() + at, 12 + xlen);
      if (!msz || msz < 12 + xlen + 8) { bz->bad = true; return false; }
      const size_t have = 12 + xlen;
      b->comp.resize(at + msz);
      if (fread(b->comp.data() + at + have, 1, msz - have, bz->fp) != msz - have) { bz->bad = true; return false; }
    } else {
      if (msz < 26) { bz->bad = true; return false; }
      b->comp.resize(at + msz);
      memcpy(b->comp.data() + at, hd, 18);
      if (fread(b->comp.data() + at + 18, 1, msz - 18, bz->fp) != msz - 18) { bz->bad = true; return false; }
    }
    const unsigned char* t = b->comp.data() + at + msz - 4;
    const size_t isz = (size_t)t[0] | ((size_t)t[1] << 8) | ((size_t)t[2] << 16) | ((size_t)t[3] << 24);
    if (isz > (1u << 16)) { bz->bad = true; return false; }
    if (isz == 0) continue;                                  // the empty end-of-file member (or an empty one in between)
    b->coff.push_back(at); b->csz.push_back(msz); b->doff.push_back(dtot);
    dtot += isz;
  }
  if (b->coff.empty()) return false;
  b->on_dev = false;
  if (bz->dev && bz->parse_on) {                                // inflated and parsed on the device; only the record tables come back
    const int rc = bz->bam ? c3_bgzf_stretch_parse_bam(bz->dev, (int)(b - bz->st), (const char*)b->comp.data(), (int64_t)b->comp.size(),
                                                       bz->carry_from, bz->carry_len, bz->bam_at_start ? 1 : 0, bz->eof ? 1 : 0, &b->fq)
                           : c3_bgzf_stretch_parse(bz->dev, (int)(b - bz->st), (const char*)b->comp.data(), (int64_t)b->comp.size(),
                                                   bz->carry_from, bz->carry_len, bz->eof ? 1 : 0, &b->fq);
    if (rc != C3_E_OK) { bz->why = c3_last_error(nullptr); bz->bad = true; return false; }
    b->on_dev = true; b->next_rec = 0; b->dend = 0;
    ++bz->n_dev;
    return true;
  }
  if (bz->parse_req) ++bz->n_host;                              // (after a departure: this stretch goes through the host parser)
  b->dec.resize(dtot);
  const size_t nm = b->coff.size();
  if (bz->dev) {                                                // one device call for the stretch; never zlib when the device was asked for
    int64_t got = 0;
    const int rc = c3_bgzf_decompress(bz->dev, (const char*)b->comp.data(), (int64_t)b->comp.size(), b->dec.data(), (int64_t)dtot, &got);
    if (rc != C3_E_OK || (size_t)got != dtot) { bz->why = c3_last_error(nullptr); bz->bad = true; return false; }
    b->dend = dtot;
    return true;
  }
  auto work = [&](size_t t0, size_t step, bool* ok) {
    for (size_t i = t0; i < nm; i += step) {
      const size_t osz = (i + 1 < nm ? b->doff[i + 1] : dtot) - b->doff[i];
      if (!bgzf_inflate(b->comp.data() + b->coff[i], b->csz[i], b->dec.data() + b->doff[i], osz)) { *ok = false; return; }
    }
  };
  const size_t nt = std::min<size_t>((size_t)std::max(1, bz->threads), nm);
  std::vector<char> oks(nt, 1);
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; ++t) th.emplace_back(work, t, nt, (bool*)&oks[t]);
  work(0, nt, (bool*)&oks[0]);
  for (auto& x : th) x.join();
  for (char o : oks) if (!o) { bz->bad = true; return false; }
  b->dend = dtot;
  return true;
}

// bytes of the inflated file, in order.  While the parser works through one stretch the next one is read and inflated on a
// thread of its own (which fans out to b->threads inflaters): the reader thread only waits when inflating is the slower side
long bgzf_read(Bgzf* b, char* dst, size_t room) {
  if (b->dpos == b->st[b->cur].dend) {
    struct Wait { Bgzf* b; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
                  ~Wait() { b->wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } } wait{b};
    if (b->pre_on) { b->pre.join(); b->pre_on = false; if (b->pre_ok) { b->cur ^= 1; b->dpos = 0; } else b->st[b->cur].dend = b->dpos = 0; }
    else { if (b->bad || !bgzf_next_stretch(b, &b->st[b->cur])) return b->bad ? -1 : 0; b->dpos = 0; }
    if (b->bad) return -1;
    if (b->st[b->cur].dend == 0) return 0;
    if (!b->eof) { BgzfStretch* nx = &b->st[b->cur ^ 1]; b->pre_on = true; b->pre = std::thread([b, nx]() { b->pre_ok = bgzf_next_stretch(b, nx); }); }
  }
  BgzfStretch& c = b->st[b->cur];
  const size_t k = std::min(room, c.dend - b->dpos);
  memcpy(dst, c.dec.data() + b->dpos, k);
  b->dpos += k;
  return (long)k;
}

bool refill(c3_reader* r) {
  if (r->eof) return false;
  if (r->beg > 0) { memmove(r->buf.data(), r->buf.data() + r->beg, r->end - r->beg); r->end -= r->beg; r->buf_off += (int64_t)r->beg; r->beg = 0; }
  if (r->end == r->buf.size()) r->buf.resize(r->buf.size() * 2);
  size_t room = r->buf.size() - r->end;
  long got = r->bz ? bgzf_read(r->bz, r->buf.data() + r->end, room)
           : r->gz ? (long)gzread(r->gz, r->buf.data() + r->end, (unsigned)std::min<size_t>(room, 1u << 30))
                   : (long)fread(r->buf.data() + r->end, 1, room, r->fp);
  if (got < 0 && r->bz) r->err = "BGZF input: a member is damaged (size, inflate or CRC)" + (r->bz->why.empty() ? std::string() : ": " + r->bz->why);
  if (got <= 0) { r->eof = true; return false; }
  r->end += (size_t)got;
  return true;
}

// next line without its terminator ('\n', optional '\r'); pointer valid until the next call
bool next_line(c3_reader* r, const char** p, size_t* len) {
  if (r->have_line) { r->have_line = false; *p = r->lp; *len = r->ll; return true; }
  size_t scanned = 0;                             // bytes from beg already known to hold no newline
  for (;;) {
    char* base = r->buf.data() + r->beg;
    const size_t avail = r->end - r->beg;
    const char* nl = (const char*)memchr(base + scanned, '\n', avail - scanned);
    if (nl) {
      size_t l = (size_t)(nl - base);
      *p = base; r->beg += l + 1;
      if (l && base[l - 1] == '\r') --l;
      *len = l;
      return true;
    }
    scanned = avail;
    if (!refill(r)) {                             // refill keeps [beg,end) intact (moved to the front)
      if (r->end > r->beg) {                      // last line without terminator
        base = r->buf.data() + r->beg;
        size_t l = r->end - r->beg;
        *p = base; r->beg = r->end;
        if (l && base[l - 1] == '\r') --l;
        *len = l;
        return true;
      }
      return false;
    }
  }
}
void unget_line(c3_reader* r, const char* p, size_t len) { r->have_line = true; r->lp = p; r->ll = len; }

int fail(c3_reader* r, const char* msg) { r->err = msg; return C3_E_ARG; }

}  // namespace

// page-locked host memory for callers that build their own batches (bench.py, tests): the same kind of buffer the reader
// hands out, so c3_batch_stage / c3_batch_upload copy it by DMA.  Plain malloc when no GPU runtime is present.
extern "C" int c3_host_alloc(int64_t bytes, void** out) {
  if (!out || bytes <= 0) return C3_E_ARG;
  HostBuf b;                                      // 64-byte header in front of the user pointer: byte 0 = page-locked?
  if (!b.reserve((size_t)bytes + 64, 0)) return C3_E_NOMEM;
  b.p[0] = b.pinned ? 1 : 0;
  *out = b.p + 64;
  b.p = nullptr; b.cap = 0;                       // ownership moves to the caller (c3_host_free)
  return C3_E_OK;
}
extern "C" void c3_host_free(void* p) {
  if (!p) return;
  char* base = (char*)p - 64;
  if (base[0]) (void)hipHostFree(base); else free(base);
}

extern "C" int c3_reader_open(const char* path, int n_sets, c3_reader** out) {
  if (!path || !out) return C3_E_ARG;
  c3_reader* r = new c3_reader();
  size_t n = strlen(path);
  r->bam = n > 4 && strcmp(path + n - 4, ".bam") == 0;
  if (r->bam || (n > 3 && strcmp(path + n - 3, ".gz") == 0)) {
    // BGZF (bgzip): members located by their headers and inflated in parallel; any other gzip file: one zlib stream.
    // A .bam is BGZF by definition (no C3_NO_BGZF escape); one that is not stays open so that the first next can say so
    unsigned char hd[18]; size_t got = 0;
    FILE* f = fopen(path, "rb");
    if (f) { got = fread(hd, 1, 18, f); }
    if (f && got == 18 && bgzf_member_size(hd, 18) && (r->bam || !getenv("C3_NO_BGZF"))) {
      rewind(f);
      r->bz = new Bgzf(); r->bz->fp = f; r->bz->bam = r->bam;
      const char* e = getenv("C3_GZ_THREADS");
      r->bz->threads = e ? std::max(1, atoi(e)) : (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    } else if (r->bam) r->fp = f;
    else {
      if (f) fclose(f);
      r->gz = gzopen(path, "rb"); if (r->gz) gzbuffer(r->gz, 1 << 20);
    }
  }
  else r->fp = fopen(path, "rb");
  if (!r->gz && !r->fp && !r->bz) { delete r; return C3_E_ARG; }
  { FILE* f = fopen(path, "rb"); if (f) { fseek(f, 0, SEEK_END); long z = ftell(f); r->file_bytes = z > 0 ? (size_t)z : 0; fclose(f); } }
  r->buf.resize((size_t)16 << 20);
  r->sets.resize((size_t)std::max(1, n_sets));
  *out = r;
  return C3_E_OK;
}

extern "C" int c3_reader_open_inflate(const char* path, int n_sets, int device, c3_reader** out) {
  if (!path || !out) return C3_E_ARG;
  *out = nullptr;
  c3_bgzf* z = nullptr;
  int rc = c3_bgzf_create(device, &z);                          // first: no usable GPU is an error whatever the file is
  if (rc != C3_E_OK) return rc;
  c3_reader* r = nullptr;
  rc = c3_reader_open(path, n_sets, &r);
  if (rc != C3_E_OK) { c3_bgzf_destroy(z); return rc; }
  if (r->bz) {
    r->bz->dev = z;
    if (const char* e = getenv("C3_INFLATE_STRETCH_MEMBERS")) { const int v = atoi(e); if (v >= 1 && v <= 4096) r->bz->stretch_members = (size_t)v; }
  } else c3_bgzf_destroy(z);                                    // plain gzip / plain text: read as c3_reader_open reads it
  *out = r;
  return C3_E_OK;
}

namespace {

// Is `p` (a line start inside [buf, buf+n)) the header of a record?  FASTA: '>' is unambiguous.  FASTQ: '@' also opens
// quality lines, so the 4-line shape is checked: '@' line, sequence, '+' line, quality of the same length as the sequence.
// Returns 1 yes, 0 no, -1 cannot tell (window too short).
int record_starts_at(const char* buf, size_t n, size_t p, bool fastq, bool at_eof = false) {
  if (p >= n) return -1;
  if (!fastq) return buf[p] == '>' ? 1 : 0;            // ('>' is also a quality character: the file's first byte decides)
  if (buf[p] != '@') return 0;
  size_t ls[5]; ls[0] = p;
  for (int k = 1; k < 5; ++k) {
    const char* nl = (const char*)memchr(buf + ls[k - 1], '\n', n - ls[k - 1]);
    if (!nl) {
      if (k == 4 && at_eof && ls[3] < n) { ls[4] = n + 1; break; }        // the file's last record without a trailing newline
      return -1;
    }
    ls[k] = (size_t)(nl - buf) + 1;
    if (k < 4 && ls[k] >= n) return -1;
  }
  if (buf[ls[2]] != '+') return 0;
  auto len = [&](int k) { size_t l = ls[k + 1] - ls[k] - 1; if (l && buf[ls[k] + l - 1] == '\r') --l; return l; };
  return len(1) == len(3) && len(1) > 0 ? 1 : 0;
}

}  // namespace

// Reader over the byte range [beg, end) of a plain (not gzip) FASTA / 4-line FASTQ file: starts at the first record that
// begins at or after `beg`, stops before the first record that begins at or after `end` -- ranges that tile the file read
// every record exactly once.  Lets every GPU worker parse its own contiguous part of the input (the reference hands 1000-read
// groups to a process pool, C3POa.py:236-256).  end < 0 = end of file.
extern "C" int c3_reader_open_range(const char* path, int n_sets, int64_t beg, int64_t end, c3_reader** out) {
  if (!path || !out || beg < 0) return C3_E_ARG;
  size_t n = strlen(path);
  if (n > 3 && strcmp(path + n - 3, ".gz") == 0) return C3_E_ARG;              // a gzip stream cannot be entered in the middle
  if (n > 4 && strcmp(path + n - 4, ".bam") == 0) return C3_E_ARG;             // ... nor a BAM file (BGZF, and records that are a linked list)
  int rc = c3_reader_open(path, n_sets, out);
  if (rc != C3_E_OK) return rc;
  c3_reader* r = *out;
  r->range_end = end;
  if (beg == 0) return C3_E_OK;
  int c0 = fgetc(r->fp);
  const bool fastq = c0 == '@';
  // resync: scan forward from beg-1 (so a record starting exactly at beg is found) for a line start that opens a record
  std::vector<char> win((size_t)8 << 20);
  int64_t at = beg - 1;
  for (;;) {
    if (fseek(r->fp, (long)at, SEEK_SET) != 0) { c3_reader_close(r); *out = nullptr; return C3_E_ARG; }
    const size_t got = fread(win.data(), 1, win.size(), r->fp);
    if (got == 0) { r->eof = true; r->buf_off = at; return C3_E_OK; }            // nothing left: an empty range
    size_t p = 0; bool found = false, grow = false;
    while (p < got) {
      const char* nl = (const char*)memchr(win.data() + p, '\n', got - p);
      if (!nl) break;
      p = (size_t)(nl - win.data()) + 1;
      if (p >= got) break;
      const int st = record_starts_at(win.data(), got, p, fastq, got < win.size());
      if (st == 1) { found = true; break; }
      if (st < 0) { grow = got == win.size(); break; }
    }
    if (found) {
      at += (int64_t)p;
      if (fseek(r->fp, (long)at, SEEK_SET) != 0) { c3_reader_close(r); *out = nullptr; return C3_E_ARG; }
      r->buf_off = at;
      if (end >= 0 && at >= end) r->eof = true;                                    // the range holds no record start
      return C3_E_OK;
    }
    if (grow && win.size() < ((size_t)1 << 30)) { win.resize(win.size() * 4); continue; }     // a record longer than the window
    if (got < win.size()) {                                                         // reached the end of the file without a record start
      // bytes but no record: not a 4-line FASTQ (multi-line records?) -- the caller must fall back to one whole-file reader
      r->eof = true; r->buf_off = at; r->range_lost = (int64_t)beg < (int64_t)r->file_bytes - 1 && got > 1; return C3_E_OK;
    }
    at += (int64_t)got - 1;                                                         // no line start decided: keep scanning
  }
}

extern "C" void c3_reader_close(c3_reader* r) {
  if (!r) return;
  if (r->gz) gzclose(r->gz);
  if (r->fp) fclose(r->fp);
  if (r->bz) { if (r->bz->pre_on) r->bz->pre.join(); if (r->bz->fp) fclose(r->bz->fp); if (r->bz->dev) c3_bgzf_destroy(r->bz->dev); delete r->bz; }
  delete r;
}

// names_only != 0: sequences and qualities are parsed (lengths, offsets and the short-read count stay exact) but not
// stored -- the first pass of C3POa.py:200-207 only needs names
extern "C" void c3_reader_names_only(c3_reader* r, int names_only) { if (r) r->names_only = names_only != 0; }

extern "C" int c3_reader_parse_on_device(c3_reader* r, int on) {
  if (!r) return C3_E_ARG;
  if (!r->bz || !r->bz->dev) { r->err = "c3_reader_parse_on_device: not a BGZF file opened by c3_reader_open_inflate"; return C3_E_STATE; }
  if (r->started) { r->err = "c3_reader_parse_on_device: after the first c3_reader_next"; return C3_E_STATE; }
  r->bz->parse_req = r->bz->parse_on = r->bz->dev_active = on != 0;
  return C3_E_OK;
}

extern "C" int c3_reader_stage_on_device(c3_reader* r, int on) {
  if (!r) return C3_E_ARG;
  if (!r->bz || !r->bz->dev || !r->bz->parse_req) { r->err = "c3_reader_stage_on_device: needs c3_reader_parse_on_device(r, 1) in force"; return C3_E_STATE; }
  if (r->started) { r->err = "c3_reader_stage_on_device: after the first c3_reader_next"; return C3_E_STATE; }
  if (on) {
    const int rc = c3_bgzf_sets_create(r->bz->dev, (int)r->sets.size());
    if (rc != C3_E_OK) { r->err = c3_last_error(nullptr); return rc; }
  }
  r->bz->stage_on = on != 0;
  return C3_E_OK;
}

extern "C" int c3_reader_device_group(const c3_reader* r, int set, c3_device_batch* out) {
  if (!r || !out || set < 0 || set >= (int)r->sets.size()) return C3_E_ARG;
  out->d_seqs = out->d_quals = nullptr; out->device = -1; out->bytes = 0;
  const BatchSet& s = r->sets[(size_t)set];
  if (!s.on_dev) return C3_E_OK;                                  // a host group (or none): no device pointers
  int dev = -1;
  const int rc = c3_bgzf_set_get(r->bz->dev, set, &out->d_seqs, &out->d_quals, &dev);
  if (rc != C3_E_OK) return rc;
  out->device = dev; out->bytes = (int64_t)s.n_bases;
  return C3_E_OK;
}

extern "C" int c3_reader_stage_stats(const c3_reader* r, int64_t* groups_device, int64_t* groups_host, int64_t* host_bytes) {
  if (!r) return C3_E_ARG;
  const Bgzf* b = r->bz;
  if (groups_device) *groups_device = b ? b->grp_dev : 0;
  if (groups_host) *groups_host = b ? b->grp_host : 0;
  if (host_bytes) *host_bytes = b ? b->host_bytes : 0;
  return C3_E_OK;
}

extern "C" int c3_reader_parse_stats(const c3_reader* r, int64_t* stretches_device, int64_t* stretches_host, int64_t* records_device) {
  if (!r) return C3_E_ARG;
  const Bgzf* b = r->bz;
  if (stretches_device) *stretches_device = b ? b->n_dev.load() : 0;
  if (stretches_host) *stretches_host = b ? b->n_host.load() : 0;
  if (records_device) *records_device = b ? b->rec_dev.load() : 0;
  return C3_E_OK;
}

extern "C" double c3_reader_inflate_wait(const c3_reader* r) { return r && r->bz ? r->bz->wait_s : 0.0; }

extern "C" const char* c3_reader_error(const c3_reader* r) { return r ? r->err.c_str() : "null reader"; }

// records without a quality line seen so far (FASTA): the reference cannot process them (C3POa.py:167 takes ord() of every
// quality character) and racon's -q 5 filter would drop every layer, so the CLI refuses such input
extern "C" int64_t c3_reader_noqual(const c3_reader* r) { return r ? r->n_noqual : 0; }
// bytes of host buffers this reader holds (diagnostic: tests/test_host_io.py checks that a tiny input stays tiny)
extern "C" int64_t c3_reader_reserved_bytes(const c3_reader* r) {
  if (!r) return 0;
  int64_t tot = 0;
  for (const BatchSet& b : r->sets) tot += (int64_t)(b.names.cap + b.seqs.cap + b.quals.cap);
  return tot;
}
// 1 when c3_reader_open_range found bytes but no record start in its range (multi-line FASTQ cannot be entered in the middle):
// the records of that range would be lost, so the caller has to read the file with ONE reader instead
extern "C" int c3_reader_range_lost(const c3_reader* r) { return r && r->range_lost ? 1 : 0; }

namespace {

// the error of a BAM reader at the record it cannot take: its index, its inflated byte offset, the reason (both paths)
int bam_fail(c3_reader* r, int reason, int64_t at) {
  char buf[320];
  snprintf(buf, sizeof buf, "BAM input: record %lld at inflated byte %lld: %s", (long long)r->n_records, (long long)at, c3_bam_reason_text(reason));
  r->err = buf;
  return C3_E_ARG;
}

// the next stretch becomes the current one (what bgzf_read does between two stretches), and the one after it starts loading.
// false: nothing more was loaded (end of file, or b->bad)
bool dev_advance(Bgzf* b) {
  struct Wait { Bgzf* b; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
                ~Wait() { b->wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } } wait{b};
  bool loaded;
  if (b->pre_on) { b->pre.join(); b->pre_on = false; loaded = b->pre_ok; if (loaded) b->cur ^= 1; }
  else { if (b->bad) return false; b->carry_from = b->carry_len = 0; loaded = bgzf_next_stretch(b, &b->st[b->cur]); }
  if (b->bad || !loaded) return false;
  BgzfStretch& c = b->st[b->cur];
  if (c.fq.info.departed) b->parse_on = false;                  // from here on the host parser (the load below already goes its way)
  b->carry_from = c.fq.info.consumed; b->carry_len = c.fq.text_bytes - c.fq.info.consumed;
  if (b->bam) {
    c.base_off = b->dev_base; b->dev_base += c.fq.info.consumed;
    if (c.fq.header_bytes > 0) b->bam_at_start = false;
    if (c.fq.info.departed) return true;                        // a departure is the reader's error: nothing more is loaded
  }
  if (!b->eof) { BgzfStretch* nx = &b->st[b->cur ^ 1]; b->pre_on = true; b->pre = std::thread([b, nx]() { b->pre_ok = bgzf_next_stretch(b, nx); }); }
  return true;
}

// First kept record (sl bases) of a reader's very first group: the bytes of max_reads records of this length, for ONE page-locked
// allocation instead of a dozen grow-and-copy steps (page-locking is slow and serialised by the driver).  The three group
// loops (device records, BAM records, text) size their first group with it; what the reader can still deliver, which caps
// it, differs between them and stays with each.
size_t first_group_estimate(int max_reads, int64_t max_bases, size_t sl) {
  size_t want = (size_t)max_reads * (sl + sl / 4) + 4096;
  if (max_bases > 0) want = std::min(want, (size_t)max_bases + sl + 4096);
  return std::min(want, (size_t)2 << 30);
}

// ... and the other buffer sets of the reader right away, `want` bytes each: a page-lock issued later, while the GPU is busy,
// stalls the running kernels for its whole duration (some 50 ms per 400 MiB).  Only as many sets as the `deliver` bytes the
// reader can still yield could fill are reserved now (a 100-read input used to pin ten buffers of max_reads reads each); the
// rest grow lazily if ever needed.  stage: the sets are the device sets of c3_reader_stage_on_device.
int reserve_other_sets(c3_reader* r, BatchSet& s, size_t want, size_t deliver, bool stage) {
  size_t left = deliver > want ? deliver - want : 0;
  for (BatchSet& o : r->sets) if (&o != &s) {
    if (left == 0) break;
    const size_t w2 = std::min(want, left + 4096);
    if (stage) { if (c3_bgzf_set_reserve(r->bz->dev, (int)(&o - r->sets.data()), (int64_t)w2, 0) != C3_E_OK) { r->err = c3_last_error(nullptr); return C3_E_NOMEM; } }
    else if (!o.seqs.reserve(w2, 0) || !o.quals.reserve(w2, 0)) return C3_E_NOMEM;
    left -= std::min(left, w2);
  }
  return C3_E_OK;
}

// the device parser's side of c3_reader_next_set: records of the device stretches enter the group under the group rule of the
// host loop below (same tests in the same order), their bytes copied from the device straight to the set's fill offsets.
// Returns with the group full, at the end of the file, or with the rest of the text handed to the host parser (a departure).
int device_fill(c3_reader* r, BatchSet& s, int max_reads, int64_t max_bases, int min_len, int* pn, size_t* pnn, size_t* pnb, int64_t* pshort) {
  Bgzf* b = r->bz;
  int n = *pn; size_t nn = *pnn, nb = *pnb; int64_t n_short = *pshort;
  int rc = C3_E_OK;
  const bool stage = b->stage_on && !r->names_only;              // the bases stay on the device, in the set of the same number
  const int set = (int)(&s - r->sets.data());
  while (n < max_reads && (max_bases <= 0 || (int64_t)nb < max_bases)) {
    BgzfStretch* c = &b->st[b->cur];
    if (!c->on_dev || c->next_rec == c->fq.info.n_kept) {
      const bool departed = c->on_dev && c->fq.info.departed;
      if (!departed && dev_advance(b)) continue;
      if (b->bad) { b->dev_active = false; break; }             // (the caller reports it)
      if (b->bam) {
        // BAM has no second parser: a departure, a record the end of the file cut and a file without a whole header are errors
        c = &b->st[b->cur];
        b->dev_active = false;
        if (departed) return bam_fail(r, c->fq.reason, c->base_off + c->fq.bad_at);
        if (b->bam_at_start) return bam_fail(r, C3_BAM_TRUNCATED, 0);
        if (c->on_dev && c->fq.text_bytes > c->fq.info.consumed) return bam_fail(r, C3_BAM_TRUNCATED, c->base_off + c->fq.info.consumed);
        c->on_dev = false; c->dend = 0; b->dpos = 0;
        r->eof = true; r->bam_hdr = true;
        break;
      }
      // a departure, or the end of the file with a record the last stretch's end cut: the text from there on goes to the
      // host parser, through the buffer bgzf_read serves
      c = &b->st[b->cur];
      const int64_t from = c->on_dev ? c->fq.info.consumed : 0;
      int64_t len = c->on_dev ? c->fq.text_bytes - from : 0;
      c->dec.resize((size_t)len);
      if (len > 0) {
        if (c3_bgzf_stretch_text(b->dev, b->cur, from, len, c->dec.data()) != C3_E_OK) { b->why = c3_last_error(nullptr); b->bad = true; len = 0; }
        else ++b->n_host;
      }
      c->on_dev = false; c->dend = (size_t)len; b->dpos = 0;
      b->parse_on = false; b->dev_active = false;
      if (len == 0 && !b->pre_on) r->eof = true;                // nothing left at all
      break;
    }
    const int64_t* off = c->fq.off; const int64_t* noff = c->fq.name_off;
    const int64_t nk = c->fq.info.n_kept;
    int64_t j = c->next_rec;
    if (off[j + 1] - off[j] < (int64_t)min_len) { ++n_short; ++r->n_records; ++b->rec_dev; c->next_rec = j + 1; continue; }
    // a run of records that all enter the group: one copy per array
    const int64_t j0 = j, sl0 = off[j + 1] - off[j];
    const size_t nn0 = nn, nb0 = nb; const int n0 = n;
    while (j < nk && n < max_reads && (max_bases <= 0 || (int64_t)nb < max_bases) && off[j + 1] - off[j] >= (int64_t)min_len) {
      nn += (size_t)(noff[j + 1] - noff[j]); nb += (size_t)(off[j + 1] - off[j]); ++n; ++j;
      s.name_off.push_back((int64_t)nn); s.off.push_back((int64_t)nb);
    }
    if (!s.names.reserve(nn + 16, nn0)) return C3_E_NOMEM;
    if (!r->names_only) {
      size_t want = nb + 16;
      if (n0 == 0 && !r->hint_bases) {
        // first kept record of the very first group: never more than the file can deliver (compressed size: a generous bound)
        const size_t deliver = r->file_bytes ? r->file_bytes * 16 + (size_t)sl0 + 4096 : (size_t)-1;
        want = std::max(want, std::min(first_group_estimate(max_reads, max_bases, (size_t)sl0), deliver));
        if (reserve_other_sets(r, s, want, deliver, stage) != C3_E_OK) return C3_E_NOMEM;
      }
      if (stage) { if (c3_bgzf_set_reserve(b->dev, set, (int64_t)want, (int64_t)nb0) != C3_E_OK) { r->err = c3_last_error(nullptr); return C3_E_NOMEM; } }
      else if (!s.seqs.reserve(want, nb0) || !s.quals.reserve(want, nb0)) return C3_E_NOMEM;
    }
    rc = stage ? c3_bgzf_stretch_stage(b->dev, b->cur, j0, j, s.names.p + nn0, set, (int64_t)nb0)
               : c3_bgzf_stretch_fetch(b->dev, b->cur, j0, j, s.names.p + nn0, r->names_only ? nullptr : s.seqs.p + nb0, r->names_only ? nullptr : s.quals.p + nb0);
    if (rc != C3_E_OK) { b->why = c3_last_error(nullptr); b->bad = true; b->dev_active = false; break; }
    r->n_records += j - j0; b->rec_dev += j - j0;
    c->next_rec = j;
  }
  *pn = n; *pnn = nn; *pnb = nb; *pshort = n_short;
  return C3_E_OK;
}

}  // namespace

// One group of reads.  Records shorter than min_len are skipped and counted in out->n_short (C3POa.py:202-204,240-241).
// Stops after max_reads kept reads or once max_bases kept bases are exceeded (0 = no limit).  out->n == 0 at end of file.
extern "C" int c3_reader_next(c3_reader* r, int max_reads, int64_t max_bases, int min_len, c3_host_batch* out) {
  if (!r) return C3_E_ARG;
  return c3_reader_next_set(r, (r->cur + 1) % (int)r->sets.size(), max_reads, max_bases, min_len, out);
}

// The same, into buffer set `set` (0 .. n_sets-1) chosen by the caller: with several consumers finishing out of order the
// caller keeps a free list of sets and hands one back only after its group has been written.
extern "C" int c3_reader_next_set(c3_reader* r, int set, int max_reads, int64_t max_bases, int min_len, c3_host_batch* out) {
  if (!r || !out || max_reads <= 0 || set < 0 || set >= (int)r->sets.size()) return C3_E_ARG;
  r->cur = set;
  BatchSet& s = r->sets[(size_t)r->cur];
  s.name_off.assign(1, 0); s.off.assign(1, 0);
  s.on_dev = false;
  // c3_reader_stage_on_device: while the device parser hands out records the group is built in the device set of this number
  const bool stage_rd = r->bz && r->bz->stage_on && !r->names_only;
  const bool try_dev = stage_rd && r->bz->dev_active;
  if (!r->names_only && r->hint_bases) {
    // later sets are allocated once, with the size the previous groups needed (growth by copying only for the first)
    const size_t want = r->hint_bases + r->hint_bases / 8 + 4096;
    if (try_dev) { if (c3_bgzf_set_reserve(r->bz->dev, set, (int64_t)want, 0) != C3_E_OK) { r->err = c3_last_error(nullptr); return C3_E_NOMEM; } }
    else if (!stage_rd && (!s.seqs.reserve(want, 0) || !s.quals.reserve(want, 0))) return C3_E_NOMEM;
  }
  size_t nn = 0, nb = 0; int n = 0; int64_t n_short = 0;
  const char* p; size_t l;
  r->started = true;
  if (r->bz && r->bz->dev_active) {                               // c3_reader_parse_on_device: the device parser fills the group ...
    const int rc = device_fill(r, s, max_reads, max_bases, min_len, &n, &nn, &nb, &n_short);
    if (rc != C3_E_OK) return rc;
  }                                                               // ... and after a departure the loop below goes on with the same group
  // ... unless it is a device group: that one ends in front of the departure (or at the end of the device's records) when it
  // holds a record; when it holds none the call goes on as an ordinary host group, in the page-locked set
  const bool dev_group = try_dev && n > 0;
  bool size_host_set = stage_rd && !dev_group && r->hint_bases;   // ... sized like a later set, but only once the text does hold a record
  // a .bam file: records by the rule of c3_bam.h (what c3_bam_parse_host applies) over the bytes bgzf_read yields
  while (r->bam && !dev_group && n < max_reads && (max_bases <= 0 || (int64_t)nb < max_bases)) {
    if (!r->bz) return fail(r, "BAM input: not a BGZF file");
    const uint8_t* d = (const uint8_t*)r->buf.data();
    const int64_t at = r->buf_off + (int64_t)r->beg;                 // inflated file offset of the record
    C3BamRec rec;
    int st;
    if (!r->bam_hdr) {
      int64_t nx = 0;
      st = c3_bam_header(d, (int64_t)r->beg, (int64_t)r->end, &nx);
      if (st == C3_BAM_OK) { r->beg = (size_t)nx; r->bam_hdr = true; continue; }
    } else st = r->beg == r->end ? (int)C3_BAM_INCOMPLETE : c3_bam_record(d, (int64_t)r->beg, (int64_t)r->end, &rec);
    if (st == C3_BAM_INCOMPLETE) {
      if (refill(r)) continue;
      if (r->bz->bad || (r->bam_hdr && r->beg == r->end)) break;     // a damaged member (reported below), or the end of the file
      return bam_fail(r, C3_BAM_TRUNCATED, r->bam_hdr ? at : 0);
    }
    if (st != C3_BAM_OK) return bam_fail(r, st, r->bam_hdr ? at : 0);
    r->beg = (size_t)rec.next;
    ++r->n_records;
    const size_t sl = rec.l_seq;
    if ((int64_t)sl < (int64_t)min_len) { ++n_short; continue; }
    if (!s.names.reserve(nn + rec.name_len + 16, nn)) return C3_E_NOMEM;
    memcpy(s.names.p + nn, d + rec.name, rec.name_len);
    if (!r->names_only) {
      size_t want = nb + sl + 16;
      if (n == 0 && !r->hint_bases) {                                // (the sizing of the text loop below: a compressed file)
        const size_t deliver = r->file_bytes ? r->file_bytes * 16 + sl + 4096 : (size_t)-1;
        want = std::max(want, std::min(first_group_estimate(max_reads, max_bases, sl), deliver));
        if (reserve_other_sets(r, s, want, deliver, false) != C3_E_OK) return C3_E_NOMEM;
      }
      if (!s.seqs.reserve(want, nb) || !s.quals.reserve(want, nb)) return C3_E_NOMEM;
      char* sq = s.seqs.p + nb; char* ql = s.quals.p + nb;
      for (size_t i = 0; i < sl; ++i) { sq[i] = (char)c3_bam_base_at(d + rec.seq, (int64_t)i); ql[i] = (char)c3_bam_qual(d[rec.qual + i]); }
    }
    nn += rec.name_len; nb += sl; ++n;
    s.name_off.push_back((int64_t)nn); s.off.push_back((int64_t)nb);
  }
  while (!r->bam && !dev_group && n < max_reads && (max_bases <= 0 || (int64_t)nb < max_bases)) {
    if (!next_line(r, &p, &l)) break;
    if (l == 0) continue;
    if (p[0] != '>' && p[0] != '@') return fail(r, "not FASTA/FASTQ: record does not start with '>' or '@'");
    if (size_host_set) {
      size_host_set = false;
      const size_t want = r->hint_bases + r->hint_bases / 8 + 4096;
      if (!s.seqs.reserve(want, 0) || !s.quals.reserve(want, 0)) return C3_E_NOMEM;
    }
    if (r->range_end >= 0 && r->buf_off + (int64_t)(p - r->buf.data()) >= r->range_end) { r->eof = true; r->beg = r->end; break; }   // next range's record
    // name = header up to the first blank (read_comment=False)
    size_t nl = 1; while (nl < l && p[nl] != ' ' && p[nl] != '\t') ++nl;
    if (!s.names.reserve(nn + nl, nn)) return C3_E_NOMEM;
    memcpy(s.names.p + nn, p + 1, nl - 1);
    const size_t name_len = nl - 1;
    // sequence lines until a line that starts with '>', '@' or '+' (kseq.h)
    const size_t sb = nb; size_t sl = 0; bool plus = false;
    while (next_line(r, &p, &l)) {
      if (l && (p[0] == '>' || p[0] == '@')) { unget_line(r, p, l); break; }
      if (l && p[0] == '+') { plus = true; break; }
      if (!r->names_only) {
        if (!s.seqs.reserve(sb + sl + l + 16, sb + sl)) return C3_E_NOMEM;
        memcpy(s.seqs.p + sb + sl, p, l);
      }
      sl += l;
    }
    if (!r->names_only && !s.quals.reserve(sb + sl + 16, sb)) return C3_E_NOMEM;
    if (plus) {
      size_t ql = 0;
      while (ql < sl && next_line(r, &p, &l)) {
        if (ql + l > sl) return fail(r, "quality string longer than the sequence");
        if (!r->names_only) memcpy(s.quals.p + sb + ql, p, l);
        ql += l;
      }
      if (ql != sl) return fail(r, "truncated quality string");
    } else {
      ++r->n_noqual;
      if (!r->names_only) memset(s.quals.p + sb, '!', sl);       // FASTA record: no qualities -> Phred 0
    }
    ++r->n_records;
    if ((int64_t)sl < (int64_t)min_len) { ++n_short; continue; }     // dropped: buffers are simply overwritten
    if (n == 0 && !r->names_only && !r->hint_bases && sl > 0) {
      // first kept record of the very first group (first_group_estimate) ...
      size_t want = first_group_estimate(max_reads, max_bases, sl);
      // ... but never more than this reader can still deliver: sequence bytes are at most half of the bytes left in its
      // file / byte range (the other half are qualities)
      size_t deliver = (size_t)-1;
      if (!r->gz && !r->bz && r->file_bytes) {
        const int64_t stop = r->range_end >= 0 ? std::min<int64_t>(r->range_end + (int64_t)(4 * sl + 4096), (int64_t)r->file_bytes) : (int64_t)r->file_bytes;
        const int64_t here = r->buf_off + (int64_t)r->beg;
        deliver = (size_t)std::max<int64_t>(0, stop - here) / 2 + sb + sl + 4096;
      } else if ((r->gz || r->bz) && r->file_bytes) deliver = r->file_bytes * 16 + sb + sl + 4096;        // (compressed size: a generous bound)
      want = std::min(want, std::max(deliver, sb + sl + 4096));
      if (!s.seqs.reserve(want, sb + sl) || !s.quals.reserve(want, sb + sl)) return C3_E_NOMEM;
      if (reserve_other_sets(r, s, want, deliver, false) != C3_E_OK) return C3_E_NOMEM;
    }
    nn += name_len; nb += sl; ++n;
    s.name_off.push_back((int64_t)nn); s.off.push_back((int64_t)nb);
  }
  if (r->bz && r->bz->bad) return fail(r, "BGZF input: a member is damaged (header, size, inflate or CRC)");      // never a silently short file
  s.n_names = nn; s.n_bases = nb;
  r->hint_bases = std::max(r->hint_bases, nb);
  out->n = n; out->n_short = n_short;
  out->names = s.names.p; out->name_off = s.name_off.data();
  out->seqs = s.seqs.p; out->quals = s.quals.p; out->off = s.off.data();
  if (dev_group) { s.on_dev = true; out->seqs = out->quals = nullptr; ++r->bz->grp_dev; }
  else if (r->bz && r->bz->stage_on && n > 0) { ++r->bz->grp_host; r->bz->host_bytes += 2 * (int64_t)nb; }
  return C3_E_OK;
}

// ---- writer ------------------------------------------------------------------------------------------------------
namespace {

// Output bytes are produced straight into slices of one pooled arena per call (kept across calls: after the first group no
// page of it is faulted in again, nothing grows by copying).  A slice is sized from an upper bound of its records, so the
// appender needs no capacity checks.
struct Out {
  char* p;
  inline void put(char c) { *p++ = c; }
  inline void app(const char* s, size_t n) { memcpy(p, s, n); p += n; }
  inline void num(long long v) {                 // decimal, no allocation
    char t[24]; int k = 0;
    unsigned long long u = v < 0 ? (unsigned long long)(-v) : (unsigned long long)v;
    do { t[k++] = (char)('0' + u % 10); u /= 10; } while (u);
    if (v < 0) *p++ = '-';
    while (k) *p++ = t[--k];
  }
};

// str(round(sum / n, 2)) of Python: correctly rounded to 2 decimals, then the shortest repr (trailing zeros dropped,
// one decimal kept) -- C3POa.py:168
void avg_qual_text(const char* q, int64_t n, Out& out) {
  unsigned long long sum = 0;
  const unsigned char* u = (const unsigned char*)q;
  for (int64_t i = 0; i < n; ++i) sum += u[i];                 // (vectorises; the -33 per base comes off afterwards)
  const long long tot = (long long)sum - 33LL * n;
  char tmp[64];
  int k = snprintf(tmp, sizeof(tmp), "%.2f", (double)tot / (double)n);
  while (k > 0 && tmp[k - 1] == '0' && k >= 2 && tmp[k - 2] != '.') --k;
  out.app(tmp, (size_t)k);
}

inline void fastq(Out& o, const char* name, size_t nl, long idx, const char* s, const char* q, int64_t b, int64_t e) {
  o.put('@'); o.app(name, nl); o.put('_'); o.num(idx); o.put('\n');
  o.app(s + b, (size_t)(e - b)); o.app("\n+\n", 3); o.app(q + b, (size_t)(e - b)); o.put('\n');
}
inline size_t fastq_bound(size_t nl, int64_t len) { return nl + 2 * (size_t)std::max<int64_t>(len, 0) + 32; }

// which records does read i produce?  (one place for the rules of C3POa.py:115-132 / determine_consensus.py:57-77,108-114)
// (the rule itself is c3_emit_of of c3_emit.h, which k_emit applies as well)
struct Emit { bool any, cons; int ns; };
inline Emit emit_of(const c3_read_result& r, int s, int n_splints, int zero, int64_t clen) {
  const C3EmitDec d = c3_emit_of(r, s, n_splints, zero, clen);
  return Emit{d.any != 0, d.cons != 0, d.ns};
}

}  // namespace

namespace {

// upper bound of the bytes reads [i0, i1) append to the consensus / subread file of every splint
void bound_range(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                 const int16_t* splint_id, int n_splints, int zero, int i0, int i1, size_t* bc, size_t* bs) {
  for (int i = i0; i < i1; ++i) {
    const c3_read_result& r = res[i];
    const int s = splint_id[i];
    const int64_t clen = cons ? cons_off[i + 1] - cons_off[i] : 0;
    const Emit e = emit_of(r, s, n_splints, zero, clen);
    if (!e.any) continue;
    const size_t nl = (size_t)(b->name_off[i + 1] - b->name_off[i]);
    const int64_t L = b->off[i + 1] - b->off[i];
    size_t q = 0;
    if (e.ns == 0) q = fastq_bound(nl, r.front_end) + fastq_bound(nl, L - r.tail_beg);
    else {
      for (int k = 0; k < e.ns; ++k) q += fastq_bound(nl, (int64_t)r.sub_end[k] - r.sub_beg[k]);
      if (r.has_front) q += fastq_bound(nl, r.front_end);
      if (r.has_tail) q += fastq_bound(nl, L - r.tail_beg);
    }
    bs[s] += q;
    if (e.cons) bc[s] += nl + (size_t)clen + 96;
  }
}

// records of reads [i0, i1) appended to oc[s] / os[s] (one slice pair per splint)
void format_range(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                  const int16_t* splint_id, int n_splints, int zero, int i0, int i1, Out* oc, Out* os) {
  for (int i = i0; i < i1; ++i) {
    const c3_read_result& r = res[i];
    const int s = splint_id[i];
    const int64_t clen = cons ? cons_off[i + 1] - cons_off[i] : 0;
    const Emit e = emit_of(r, s, n_splints, zero, clen);
    if (!e.any) continue;
    const char* name = b->names + b->name_off[i]; const size_t nl = (size_t)(b->name_off[i + 1] - b->name_off[i]);
    const char* seq = b->seqs + b->off[i]; const char* qual = b->quals + b->off[i];
    const int64_t L = b->off[i + 1] - b->off[i];
    const int ns = e.ns;
    Out& fq = os[s];
    if (ns == 0) {
      fastq(fq, name, nl, 0, seq, qual, 0, r.front_end);
      fastq(fq, name, nl, 1, seq, qual, r.tail_beg, L);
    } else {
      for (int k = 0; k < ns; ++k) fastq(fq, name, nl, k + 1, seq, qual, r.sub_beg[k], r.sub_end[k]);
      int j = 0;
      if (r.has_front) { fastq(fq, name, nl, 0, seq, qual, 0, r.front_end); ++j; }
      if (r.has_tail) fastq(fq, name, nl, j == 0 ? 0 : ns + 1, seq, qual, r.tail_beg, L);
    }
    if (e.cons) {
      Out& fa = oc[s];
      fa.put('>'); fa.app(name, nl); fa.put('_');
      avg_qual_text(qual, L, fa);
      fa.put('_'); fa.num((long long)L); fa.put('_'); fa.num(ns);
      fa.put('_'); fa.num((long long)clen); fa.put('\n');
      fa.app(cons + cons_off[i], (size_t)clen); fa.put('\n');
    }
  }
}

// pooled arenas: one per c3_write_group call in flight, grow-only, reused by later calls
struct Arena { char* p = nullptr; size_t cap = 0; };
std::mutex g_arena_mu;
std::vector<Arena> g_arena_free;
Arena arena_get(size_t need) {
  Arena a;
  {
    std::lock_guard<std::mutex> lk(g_arena_mu);
    size_t best = (size_t)-1;
    for (size_t k = 0; k < g_arena_free.size(); ++k)
      if (g_arena_free[k].cap >= need && (best == (size_t)-1 || g_arena_free[k].cap < g_arena_free[best].cap)) best = k;
    if (best == (size_t)-1 && !g_arena_free.empty()) best = 0;                 // too small: take one and grow it
    if (best != (size_t)-1) { a = g_arena_free[best]; g_arena_free.erase(g_arena_free.begin() + (long)best); }
  }
  if (a.cap < need) { free(a.p); a.cap = need + need / 8 + 4096; a.p = (char*)malloc(a.cap); if (!a.p) a.cap = 0; }
  return a;
}
void arena_put(Arena a) { if (a.p) { std::lock_guard<std::mutex> lk(g_arena_mu); g_arena_free.push_back(a); } }

bool pwrite_all(int fd, const char* p, size_t n, off_t at) {
  while (n) {
    ssize_t w = pwrite(fd, p, n, at);
    if (w < 0) { if (errno == EINTR) continue; return false; }
    p += w; n -= (size_t)w; at += w;
  }
  return true;
}

}  // namespace

// Appends the records of one group to <cons_paths[s]> / <sub_paths[s]> (s = splint_id[i]; reads with splint_id < 0 or a
// status that produces no output are skipped).  Record formats and the subread naming asymmetry follow the reference:
// kept subreads _1.._n, first dangling piece _0, second _<n+1> (determine_consensus.py:57-62,69-77); zero-repeat pieces
// _0,_1 are written before the rescue is tried (:108-114); consensus header name_avgQ_rawLen_repeats_consLen (C3POa.py:168-171).
// The group is cut into contiguous read ranges that are formatted and written (pwrite at precomputed offsets) by a few
// threads: record order in the files is read order, exactly as with one thread.
namespace {
// Append reservations per output file: a group's bytes go to [at, at + total) of the file, where `at` is handed out under a
// lock, so the writer threads of several GPU workers can format and pwrite into ONE file concurrently (no part files, no
// merge pass).  c3_writer_reset forgets the table (the caller truncates its files at the start of a run).
std::mutex g_res_mu;
struct ResEntry { off_t next = 0; int inflight = 0; };
struct ResKey { dev_t dev; ino_t ino; bool operator==(const ResKey& o) const { return dev == o.dev && ino == o.ino; } };
struct ResKeyHash { size_t operator()(const ResKey& k) const { return std::hash<unsigned long long>()((unsigned long long)k.dev * 1000003ull ^ (unsigned long long)k.ino); } };
// keyed by the FILE (device, inode), not by the path string: two spellings of one path share one entry, a replaced file
// gets a new one.  An entry only lives while reservations are in flight: once the last writer of a file has finished, the
// next group starts again from the file's real end, so a file truncated between calls is not extended with a hole.
std::unordered_map<ResKey, ResEntry, ResKeyHash> g_res;
bool res_key(int fd, ResKey* k) { struct stat st; if (fstat(fd, &st) != 0) return false; k->dev = st.st_dev; k->ino = st.st_ino; return true; }
off_t reserve_append(int fd, size_t total) {
  std::lock_guard<std::mutex> lk(g_res_mu);
  const off_t end = lseek(fd, 0, SEEK_END);
  ResKey k;
  if (!res_key(fd, &k)) return end;
  ResEntry& e = g_res[k];
  const off_t at = e.inflight > 0 ? std::max(end, e.next) : end;
  e.next = at + (off_t)total; e.inflight++;
  return at;
}
void release_append(int fd) {
  std::lock_guard<std::mutex> lk(g_res_mu);
  ResKey k;
  if (!res_key(fd, &k)) return;
  auto it = g_res.find(k);
  if (it != g_res.end() && --it->second.inflight <= 0) g_res.erase(it);
}
}  // namespace

extern "C" void c3_writer_reset(void) { std::lock_guard<std::mutex> lk(g_res_mu); g_res.clear(); }

namespace {
// phases 0 and 1 of a writer call: the group cut into T contiguous read ranges, each range's records formatted (in
// parallel) into its own (kind, splint) slices of one pooled arena.  Slice x = k * NS + s of thread k: consensus text
// [sc[x], oc[x].p), subread text [ss[x], os[x].p).
struct Formatted {
  int T = 1; size_t NS = 0; Arena ar;
  std::vector<char*> sc, ss; std::vector<Out> oc, os;
  template <class F> void run_all(F&& fn) const {
    std::vector<std::thread> th;
    for (int k = 0; k < T; ++k) { if (k + 1 < T) th.emplace_back(fn, k); else fn(k); }
    for (auto& x : th) x.join();
  }
  size_t len(int kind, size_t x) const { return kind ? (size_t)(os[x].p - ss[x]) : (size_t)(oc[x].p - sc[x]); }
  const char* txt(int kind, size_t x) const { return kind ? ss[x] : sc[x]; }
};
int format_group(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                 const int16_t* splint_id, int n_splints, int zero, Formatted& f) {
  int T = 1;
  if (b->n >= 4096) { T = 8; if (const char* e = getenv("C3_WRITER_THREADS")) T = std::max(1, std::min(64, atoi(e))); }
  f.T = T;
  const size_t NS = f.NS = (size_t)n_splints;
  auto range = [&](int k, int* i0, int* i1) { *i0 = (int)((int64_t)b->n * k / T); *i1 = (int)((int64_t)b->n * (k + 1) / T); };
  // phase 0: size of every (thread, kind, splint) slice from an upper bound of its records; one pooled arena holds them all
  std::vector<size_t> bc((size_t)T * NS, 0), bs((size_t)T * NS, 0);
  f.run_all([&](int k) { int i0, i1; range(k, &i0, &i1); bound_range(b, res, cons, cons_off, splint_id, n_splints, zero, i0, i1, &bc[(size_t)k * NS], &bs[(size_t)k * NS]); });
  size_t need = 64;
  for (size_t x : bc) need += x;
  for (size_t x : bs) need += x;
  f.ar = arena_get(need);
  if (!f.ar.p) return C3_E_NOMEM;
  f.sc.resize((size_t)T * NS); f.ss.resize((size_t)T * NS);             // slice starts
  { char* p = f.ar.p; for (size_t x = 0; x < (size_t)T * NS; ++x) { f.sc[x] = p; p += bc[x]; f.ss[x] = p; p += bs[x]; } }
  f.oc.resize((size_t)T * NS); f.os.resize((size_t)T * NS);
  for (size_t x = 0; x < (size_t)T * NS; ++x) { f.oc[x].p = f.sc[x]; f.os[x].p = f.ss[x]; }
  // phase 1: format (parallel), straight into the slices
  f.run_all([&](int k) { int i0, i1; range(k, &i0, &i1); format_range(b, res, cons, cons_off, splint_id, n_splints, zero, i0, i1, &f.oc[(size_t)k * NS], &f.os[(size_t)k * NS]); });
  return C3_E_OK;
}

// R2C2_Consensus.fastq text of splint s (the consensus records of c3_write_group, emit_of, same header, with the QV line)
size_t format_consensus_fastq(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                              const char* qv, const int16_t* splint_id, int n_splints, int zero, int s, char* buf) {
  Out o{buf};
  for (int i = 0; i < b->n; ++i) {
    if (splint_id[i] != s) continue;
    const int64_t clen = cons_off[i + 1] - cons_off[i];
    const Emit e = emit_of(res[i], s, n_splints, zero, clen);
    if (!e.cons) continue;
    const char* name = b->names + b->name_off[i]; const size_t nl = (size_t)(b->name_off[i + 1] - b->name_off[i]);
    const int64_t L = b->off[i + 1] - b->off[i];
    o.put('@'); o.app(name, nl); o.put('_');
    avg_qual_text(b->quals + b->off[i], L, o);
    o.put('_'); o.num((long long)L); o.put('_'); o.num(e.ns);
    o.put('_'); o.num((long long)clen); o.put('\n');
    o.app(cons + cons_off[i], (size_t)clen); o.app("\n+\n", 3);
    o.app(qv + cons_off[i], (size_t)clen); o.put('\n');
  }
  return (size_t)(o.p - buf);
}
std::vector<size_t> consensus_fastq_bounds(const c3_host_batch* b, const c3_read_result* res, const int64_t* cons_off,
                                           const int16_t* splint_id, int n_splints, int zero) {
  std::vector<size_t> bound((size_t)n_splints, 0);
  for (int i = 0; i < b->n; ++i) {
    const int64_t clen = cons_off[i + 1] - cons_off[i];
    const Emit e = emit_of(res[i], splint_id[i], n_splints, zero, clen);
    if (e.cons) bound[(size_t)splint_id[i]] += (size_t)(b->name_off[i + 1] - b->name_off[i]) + 2 * (size_t)clen + 96;
  }
  return bound;
}

// compressed bytes of one file: appended at a reserved range of the compressed file, by T threads (one contiguous piece each,
// as c3_write_group's phase 2 does)
bool append_file(const char* path, const char* p, size_t n, const Formatted* f = nullptr) {
  const int fd = open(path, O_WRONLY | O_CREAT, 0644);
  if (fd < 0) return false;
  const off_t at = reserve_append(fd, n);
  bool ok = true;
  if (f && f->T > 1 && n >= ((size_t)1 << 20)) {
    const int T = f->T;
    std::vector<char> good((size_t)T, 1);
    f->run_all([&](int k) {
      const size_t b = n * (size_t)k / (size_t)T, e = n * (size_t)(k + 1) / (size_t)T;
      if (!pwrite_all(fd, p + b, e - b, at + (off_t)b)) good[(size_t)k] = 0;
    });
    for (char g : good) ok = ok && g;
  } else {
    ok = pwrite_all(fd, p, n, at);
  }
  release_append(fd);
  if (close(fd) != 0) ok = false;
  return ok;
}
}  // namespace

extern "C" int c3_bgzf_compress_pieces(c3_bgzf* z, const char* const* p, const int64_t* len, int np, char* dst, int64_t cap, int64_t* out_len);

extern "C" int c3_write_group(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                              const int16_t* splint_id, int n_splints, const char* const* cons_paths,
                              const char* const* sub_paths, int zero) {
  if (!b || !res || !cons_off || !splint_id || n_splints <= 0 || !cons_paths || !sub_paths) return C3_E_ARG;
  Formatted f;
  int rc = format_group(b, res, cons, cons_off, splint_id, n_splints, zero, f);
  if (rc) return rc;
  const int T = f.T; const size_t NS = f.NS;
  if (getenv("C3_WRITER_NO_IO")) { arena_put(f.ar); return C3_E_OK; }      // diagnostic (tools/formatter_throughput.py): the formatter alone
  // phase 2: one pwrite stream per (thread, file), offsets from the current file size
  struct Job { int fd; const char* txt; size_t len; off_t at; };
  std::vector<std::vector<Job>> jobs((size_t)T);
  std::vector<int> fds;
  bool ok = true;
  for (int s = 0; s < n_splints && ok; ++s) {
    for (int kind = 0; kind < 2 && ok; ++kind) {
      const char* path = kind ? sub_paths[s] : cons_paths[s];
      size_t total = 0;
      for (int k = 0; k < T; ++k) total += f.len(kind, (size_t)k * NS + (size_t)s);
      if (!total || !path) continue;
      int fd = open(path, O_WRONLY | O_CREAT, 0644);
      if (fd < 0) { ok = false; break; }
      fds.push_back(fd);
      off_t at = reserve_append(fd, total);                 // several writer threads (one per GPU worker) append to one file
      for (int k = 0; k < T; ++k) {
        const size_t x = (size_t)k * NS + (size_t)s;
        const size_t len = f.len(kind, x);
        if (len) { jobs[(size_t)k].push_back({fd, f.txt(kind, x), len, at}); at += (off_t)len; }
      }
    }
  }
  if (ok) {
    std::vector<char> good((size_t)T, 1);
    f.run_all([&](int k) { for (const Job& j : jobs[(size_t)k]) if (!pwrite_all(j.fd, j.txt, j.len, j.at)) good[(size_t)k] = 0; });
    for (char g : good) ok = ok && g;
  }
  arena_put(f.ar);
  for (int fd : fds) { release_append(fd); if (close(fd) != 0) ok = false; }
  return ok ? C3_E_OK : C3_E_ARG;
}

// --bgzf: the same slices; each file's text of the call (its T slices in record order) is compressed through z as one text
// (the slices land back to back on the device), so the members do not depend on C3_WRITER_THREADS
extern "C" int c3_write_group_bgzf(c3_bgzf* z, const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                                   const int16_t* splint_id, int n_splints, const char* const* cons_paths,
                                   const char* const* sub_paths, int zero) {
  if (!z || !b || !res || !cons_off || !splint_id || n_splints <= 0 || !cons_paths || !sub_paths) return C3_E_ARG;
  Formatted f;
  int rc = format_group(b, res, cons, cons_off, splint_id, n_splints, zero, f);
  if (rc) return rc;
  const int T = f.T; const size_t NS = f.NS;
  std::vector<const char*> pp((size_t)T);
  std::vector<int64_t> pl((size_t)T);
  Arena zb;
  for (int s = 0; s < n_splints && rc == C3_E_OK; ++s) {
    for (int kind = 0; kind < 2 && rc == C3_E_OK; ++kind) {
      const char* path = kind ? sub_paths[s] : cons_paths[s];
      int64_t total = 0;
      for (int k = 0; k < T; ++k) { const size_t x = (size_t)k * NS + (size_t)s; pp[(size_t)k] = f.txt(kind, x); pl[(size_t)k] = (int64_t)f.len(kind, x); total += pl[(size_t)k]; }
      if (!total || !path) continue;
      const int64_t cap = c3_bgzf_bound(total);
      if (zb.cap < (size_t)cap) { arena_put(zb); zb = arena_get((size_t)cap); if (!zb.p) { rc = C3_E_NOMEM; break; } }
      int64_t clen = 0;
      rc = c3_bgzf_compress_pieces(z, pp.data(), pl.data(), T, zb.p, (int64_t)zb.cap, &clen);
      if (rc == C3_E_OK && !append_file(path, zb.p, (size_t)clen, &f)) rc = C3_E_ARG;
    }
  }
  arena_put(zb);
  arena_put(f.ar);
  return rc;
}

// R2C2_Consensus.fastq beside the FASTA: the consensus records of c3_write_group (emit_of, same header) with the QV line.
// One formatting pass per splint file (the records are a small share of the group's bytes), then c3_write_group's
// reservation of the byte range at the end of the file and one pwrite.
extern "C" int c3_write_consensus_fastq(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                                        const char* qv, const int16_t* splint_id, int n_splints, const char* const* fq_paths, int zero) {
  if (!b || !res || !cons || !cons_off || !qv || !splint_id || n_splints <= 0 || !fq_paths) return C3_E_ARG;
  const std::vector<size_t> bound = consensus_fastq_bounds(b, res, cons_off, splint_id, n_splints, zero);
  bool ok = true;
  for (int s = 0; s < n_splints && ok; ++s) {
    if (!bound[(size_t)s] || !fq_paths[s]) continue;
    std::vector<char> buf(bound[(size_t)s]);
    const size_t total = format_consensus_fastq(b, res, cons, cons_off, qv, splint_id, n_splints, zero, s, buf.data());
    if (!total) continue;
    const int fd = open(fq_paths[s], O_WRONLY | O_CREAT, 0644);
    if (fd < 0) { ok = false; break; }
    const off_t at = reserve_append(fd, total);
    if (!pwrite_all(fd, buf.data(), total, at)) ok = false;
    release_append(fd);
    if (close(fd) != 0) ok = false;
  }
  return ok ? C3_E_OK : C3_E_ARG;
}

extern "C" int c3_write_consensus_fastq_bgzf(c3_bgzf* z, const c3_host_batch* b, const c3_read_result* res, const char* cons,
                                             const int64_t* cons_off, const char* qv, const int16_t* splint_id, int n_splints,
                                             const char* const* fq_paths, int zero) {
  if (!z || !b || !res || !cons || !cons_off || !qv || !splint_id || n_splints <= 0 || !fq_paths) return C3_E_ARG;
  const std::vector<size_t> bound = consensus_fastq_bounds(b, res, cons_off, splint_id, n_splints, zero);
  int rc = C3_E_OK;
  for (int s = 0; s < n_splints && rc == C3_E_OK; ++s) {
    if (!bound[(size_t)s] || !fq_paths[s]) continue;
    std::vector<char> buf(bound[(size_t)s]);
    const int64_t total = (int64_t)format_consensus_fastq(b, res, cons, cons_off, qv, splint_id, n_splints, zero, s, buf.data());
    if (!total) continue;
    std::vector<char> zbuf((size_t)c3_bgzf_bound(total));
    int64_t clen = 0;
    rc = c3_bgzf_compress(z, buf.data(), total, zbuf.data(), (int64_t)zbuf.size(), &clen);
    if (rc == C3_E_OK && !append_file(fq_paths[s], zbuf.data(), (size_t)clen)) rc = C3_E_ARG;
  }
  return rc;
}

// --emit gpu: finished streams (c3_emit_group, c3_batch_emit_fetch) appended to their files with the writers' reservation
extern "C" int c3_append_streams(const char* const* paths, const char* arena, const int64_t* stream_off, int n_streams) {
  if (!paths || !stream_off || n_streams < 0) return C3_E_ARG;
  for (int x = 0; x < n_streams; ++x) if (stream_off[x + 1] < stream_off[x] || stream_off[0] < 0) return C3_E_ARG;
  if (n_streams > 0 && stream_off[n_streams] > stream_off[0] && !arena) return C3_E_ARG;
  for (int x = 0; x < n_streams; ++x) {
    const int64_t len = stream_off[x + 1] - stream_off[x];
    if (!len || !paths[x]) continue;
    if (!append_file(paths[x], arena + stream_off[x], (size_t)len)) {      // (the code c3_write_group and its kin return for I/O errors, with the reason)
      const int err = errno;
      char msg[512];
      snprintf(msg, sizeof msg, "c3_append_streams: stream %d: cannot append %lld bytes to %s: %s", x, (long long)len, paths[x], strerror(err));
      c3_set_host_error(msg);
      return C3_E_ARG;
    }
  }
  return C3_E_OK;
}

// ---- oligo-dT index matcher of the post-processing step (C3POa_postprocessing.py:266-285, match_index) ----------
// seq is slid over every index (file order); the Levenshtein distance of seq[p : p+len(idx)] to idx is taken for every
// position where the slice has the full length (at a position where it is too short for index k the reference breaks
// out of the loop over indexes, so k+1.. are skipped there as well); per index the minimum counts.  Stable sort by
// distance; the best index wins when its distance is < 2 and the runner-up is more than 1 further away.  Returns the
// winning index number, -1 for '-'.  (The reference raises on an index that never fits and on fewer than two indexes;
// both cases return -1 here.)
namespace {
int edit_distance(const char* a, const char* b, int n) {
  int prev[256], cur[256];
  if (n > 255) return n;
  for (int j = 0; j <= n; ++j) prev[j] = j;
  for (int i = 1; i <= n; ++i) {
    cur[0] = i;
    for (int j = 1; j <= n; ++j) {
      int v = prev[j - 1] + (a[i - 1] != b[j - 1]);
      v = std::min(v, prev[j] + 1); v = std::min(v, cur[j - 1] + 1);
      cur[j] = v;
    }
    memcpy(prev, cur, sizeof(int) * (size_t)(n + 1));
  }
  return prev[n];
}
}  // namespace

extern "C" int c3_match_index(const char* seq, int n, int n_idx, const char* idx_cat, const int64_t* idx_off) {
  if (!seq || n_idx < 2 || !idx_cat || !idx_off) return -1;
  std::vector<int> best((size_t)n_idx, INT32_MAX);
  for (int p = 0; p < n; ++p) {
    for (int k = 0; k < n_idx; ++k) {
      const int len = (int)(idx_off[k + 1] - idx_off[k]);
      if (p + len > n) break;                                   // the reference's `break` (not `continue`)
      best[(size_t)k] = std::min(best[(size_t)k], edit_distance(seq + p, idx_cat + idx_off[k], len));
    }
  }
  int i0 = -1, i1 = -1;                                         // first and second entry of the stable sort
  for (int k = 0; k < n_idx; ++k) {
    if (best[(size_t)k] == INT32_MAX) return -1;
    if (i0 < 0 || best[(size_t)k] < best[(size_t)i0]) { i1 = i0; i0 = k; }
    else if (i1 < 0 || best[(size_t)k] < best[(size_t)i1]) i1 = k;
  }
  if (best[(size_t)i0] < 2 && best[(size_t)i1] - best[(size_t)i0] > 1) return i0;
  return -1;
}

// ---- sample demultiplexer (paper/Demultiplex_R2C2_reads.py, demultiplex) ------------------------------------------
// c3_demux_prepare checks the two index sets for both entry points and builds the byte -> code table of k_demux: the
// distinct bytes of all indexes get codes 1..K in byte order, every other byte 0 (which matches no index position).
int c3_demux_prepare(int n_a, const char* a_cat, const int64_t* a_off, int n_b, const char* b_cat, const int64_t* b_off,
                     uint8_t* tab, int* n_codes, const char** msg) {
  const int ns[2] = {n_a, n_b}; const char* cats[2] = {a_cat, b_cat}; const int64_t* offs[2] = {a_off, b_off};
  bool seen[256] = {};
  for (int s = 0; s < 2; ++s) {
    if (ns[s] < 2) { *msg = "an index set needs at least 2 indexes (the reference compares the best with the runner-up)"; return C3_E_ARG; }
    if (ns[s] > C3_DEMUX_MAX_IDX) { *msg = "more than 128 indexes in one set"; return C3_E_LIMIT; }
    if (!offs[s] || offs[s][0] != 0) { *msg = "index offsets missing or not starting at 0"; return C3_E_ARG; }
    for (int k = 0; k < ns[s]; ++k) {
      const int64_t len = offs[s][k + 1] - offs[s][k];
      if (len < 0) { *msg = "index offsets decrease"; return C3_E_ARG; }
      if (len > C3_DEMUX_MAX_LEN) { *msg = "index longer than 32 bytes"; return C3_E_LIMIT; }
      if (len > 0 && !cats[s]) { *msg = "index bytes missing"; return C3_E_ARG; }
      for (int64_t j = 0; j < len; ++j) seen[(uint8_t)cats[s][offs[s][k] + j]] = true;
    }
  }
  int K = 0;
  for (int b = 0; b < 256; ++b) tab[b] = seen[b] ? (uint8_t)++K : 0;
  if (K > C3_DEMUX_MAX_BYTES) { *msg = "more than 31 distinct bytes over the index sets"; return C3_E_LIMIT; }
  *n_codes = K;
  return C3_E_OK;
}

// Host statement of k_demux: textbook DP for every window (head[i : i+m], i < 300 - m) of every index.
extern "C" int c3_demux_host(int n, const char* heads, int n_a, const char* a_cat, const int64_t* a_off,
                             int n_b, const char* b_cat, const int64_t* b_off, int32_t* win, uint8_t* dist) {
  if (n < 0 || (n > 0 && (!heads || !win))) { c3_set_host_error("heads / win missing"); return C3_E_ARG; }
  uint8_t tab[256]; int K = 0; const char* msg = "";
  const int rc = c3_demux_prepare(n_a, a_cat, a_off, n_b, b_cat, b_off, tab, &K, &msg);
  if (rc != C3_E_OK) { c3_set_host_error(msg); return rc; }
  const int ns[2] = {n_a, n_b}; const char* cats[2] = {a_cat, b_cat}; const int64_t* offs[2] = {a_off, b_off};
  std::vector<int> d((size_t)std::max(n_a, n_b));
  for (int r = 0; r < n; ++r) {
    const char* head = heads + (size_t)r * C3_DEMUX_HEAD;
    for (int s = 0; s < 2; ++s) {
      for (int k = 0; k < ns[s]; ++k) {
        const int m = (int)(offs[s][k + 1] - offs[s][k]);
        int best = m;                                           // an empty index: distance 0
        for (int i = 0; i < C3_DEMUX_HEAD - m; ++i) best = std::min(best, edit_distance(cats[s] + offs[s][k], head + i, m));
        d[(size_t)k] = best;
        if (dist) dist[(size_t)r * (n_a + n_b) + (s ? n_a : 0) + k] = (uint8_t)best;
      }
      int i0 = 0;                                               // first entry of the stable sort; the runner-up's distance
      for (int k = 1; k < ns[s]; ++k) if (d[(size_t)k] < d[(size_t)i0]) i0 = k;
      int d1 = INT32_MAX;
      for (int k = 0; k < ns[s]; ++k) if (k != i0) d1 = std::min(d1, d[(size_t)k]);
      win[2 * (size_t)r + s] = (d[(size_t)i0] < 4 && d[(size_t)i0] < d1 - 1) ? i0 : -1;
    }
  }
  return C3_E_OK;
}

// ---- splint assignment from the PSL (bin/preprocess.py:22-45) without per-read Python objects ---------------------
// Rows with qBaseInsert (col 5) < 50 and matches (col 0) > 50 count; per read the row with the most matches wins, the
// earliest row on ties (Python's stable sort with reverse=True keeps the first of equal keys); every splint named by a
// counted row is "seen" (adapter_set).  Rows naming a splint that is not in the splint file are ignored.
#include <unordered_map>

struct c3_assign {
  // open-addressing table keyed by the read name: names live in one arena (no per-row allocation), rows are parsed by several
  // threads and inserted in file order (3 M rows: 2.1 s through std::unordered_map<std::string, ...>, ~0.4 s like this)
  struct Slot { uint64_t hash; uint32_t name_off, name_len; float matches; int16_t splint; char strand; char used; };
  std::vector<Slot> slots; size_t mask = 0, n_used = 0;
  std::vector<char> names;
  std::unordered_map<std::string, int> splint_of;
  std::vector<uint8_t> seen;
  int64_t rows_kept = 0;
  static uint64_t hash_of(const char* p, size_t n) { uint64_t h = 1469598103934665603ull; for (size_t i = 0; i < n; ++i) { h ^= (unsigned char)p[i]; h *= 1099511628211ull; } return h | 1; }
  void grow() {
    std::vector<Slot> old; old.swap(slots);
    slots.assign(old.empty() ? (size_t)1 << 16 : old.size() * 2, Slot{0, 0, 0, 0.f, 0, 0, 0});
    mask = slots.size() - 1;
    for (const Slot& o : old) if (o.used) { size_t i = (size_t)o.hash & mask; while (slots[i].used) i = (i + 1) & mask; slots[i] = o; }
  }
  Slot* find(const char* p, size_t n, uint64_t h) {
    if (slots.empty()) return nullptr;
    for (size_t i = (size_t)h & mask;; i = (i + 1) & mask) {
      Slot& s = slots[i];
      if (!s.used) return nullptr;
      if (s.hash == h && s.name_len == n && memcmp(names.data() + s.name_off, p, n) == 0) return &s;
    }
  }
  void upsert(const char* p, size_t n, float matches, int16_t splint, char strand) {
    const uint64_t h = hash_of(p, n);
    if (Slot* s = find(p, n, h)) { if (matches > s->matches) { s->matches = matches; s->splint = splint; s->strand = strand; } return; }   // earliest row wins ties
    if ((n_used + 1) * 10 > slots.size() * 6) grow();
    size_t i = (size_t)h & mask;
    while (slots[i].used) i = (i + 1) & mask;
    slots[i] = Slot{h, (uint32_t)names.size(), (uint32_t)n, matches, splint, strand, 1};
    names.insert(names.end(), p, p + n);
    ++n_used;
  }
};

namespace {
struct PslRow { const char* name; uint32_t name_len; float matches; int16_t splint; char strand; };
// rows of [p, e) (whole lines) that count (bin/preprocess.py:32: qBaseInsert < 50 and matches > 50) and name a known splint
void parse_psl_chunk(const char* p, const char* e, const std::unordered_map<std::string, int>& splint_of, std::vector<PslRow>& out) {
  std::string key;
  while (p < e) {
    const char* nl = (const char*)memchr(p, '\n', (size_t)(e - p));
    const char* le = nl ? nl : e;
    const char* lend = le;
    while (lend > p && (lend[-1] == '\r' || lend[-1] == '\n')) --lend;
    if (lend > p) {
      const char* col[21]; size_t len[21]; int nc = 0;
      const char* q = p;
      while (nc < 21) {
        const char* t = (const char*)memchr(q, '\t', (size_t)(lend - q));
        col[nc] = q; len[nc] = t ? (size_t)(t - q) : (size_t)(lend - q); ++nc;
        if (!t) break;
        q = t + 1;
      }
      if (nc >= 14) {
        char tmp[64];
        auto num = [&](int c) { size_t l = std::min(len[c], sizeof(tmp) - 1); memcpy(tmp, col[c], l); tmp[l] = 0; return strtod(tmp, nullptr); };
        const double matches = num(0), gaps = num(5);
        if (gaps < 50 && matches > 50) {
          key.assign(col[13], len[13]);
          auto sp = splint_of.find(key);
          if (sp != splint_of.end()) out.push_back(PslRow{col[9], (uint32_t)len[9], (float)matches, (int16_t)sp->second, len[8] ? col[8][0] : '?'});
        }
      }
    }
    p = nl ? nl + 1 : e;
  }
}
}  // namespace

extern "C" int c3_assign_open(const char* psl_path, int n_splints, const char* const* splint_names, c3_assign** out) {
  if (!psl_path || n_splints <= 0 || !splint_names || !out) return C3_E_ARG;
  FILE* f = fopen(psl_path, "rb");
  if (!f) return C3_E_ARG;
  c3_assign* a = new c3_assign();
  for (int i = 0; i < n_splints; ++i) a->splint_of.emplace(splint_names[i], i);
  a->seen.assign((size_t)n_splints, 0);
  a->grow();
  // the file goes through in slabs of whole lines; every slab is cut at line boundaries into one chunk per thread
  const size_t SLAB = (size_t)256 << 20;
  std::vector<char> buf(SLAB + 1);
  size_t have = 0;
  int T = 8; if (const char* e = getenv("C3_PSL_THREADS")) T = std::max(1, std::min(64, atoi(e)));
  for (;;) {
    const size_t got = fread(buf.data() + have, 1, SLAB - have, f);
    const bool last = got == 0 || have + got < SLAB;
    size_t n = have + got;
    size_t use = n;
    if (!last) { while (use > 0 && buf[use - 1] != '\n') --use; if (use == 0) { buf.resize(buf.size() * 2); have = n; continue; } }   // (a line longer than the slab)
    if (use > 0) {
      std::vector<std::vector<PslRow>> rows((size_t)T);
      std::vector<size_t> cut((size_t)T + 1, use);
      cut[0] = 0;
      for (int k = 1; k < T; ++k) { size_t c = use * (size_t)k / (size_t)T; while (c < use && c > 0 && buf[c - 1] != '\n') ++c; cut[(size_t)k] = std::max(c, cut[(size_t)k - 1]); }
      std::vector<std::thread> th;
      for (int k = 0; k < T; ++k) {
        auto fn = [&, k]() { parse_psl_chunk(buf.data() + cut[(size_t)k], buf.data() + cut[(size_t)k + 1], a->splint_of, rows[(size_t)k]); };
        if (k + 1 < T) th.emplace_back(fn); else fn();
      }
      for (auto& x : th) x.join();
      for (int k = 0; k < T; ++k)                                            // file order: the earliest row keeps a tie
        for (const PslRow& r : rows[(size_t)k]) { a->seen[(size_t)r.splint] = 1; ++a->rows_kept; a->upsert(r.name, r.name_len, r.matches, r.splint, r.strand); }
    }
    if (last) break;
    memmove(buf.data(), buf.data() + use, n - use);
    have = n - use;
  }
  fclose(f);
  *out = a;
  return C3_E_OK;
}

extern "C" void c3_assign_close(c3_assign* a) { delete a; }

// splint row / strand of every read of the group: -1 / '?' when the read has no counted row.  Returns the number of
// assigned reads (>= 0) or a negative c3_err.
extern "C" int c3_assign_batch(const c3_assign* a, const c3_host_batch* b, int16_t* splint_id, char* strand) {
  if (!a || !b || !splint_id || !strand) return C3_E_ARG;
  int n_ok = 0;
  c3_assign* m = const_cast<c3_assign*>(a);                                 // (find() does not modify)
  for (int i = 0; i < b->n; ++i) {
    const char* p = b->names + b->name_off[i]; const size_t n = (size_t)(b->name_off[i + 1] - b->name_off[i]);
    const c3_assign::Slot* s = m->find(p, n, c3_assign::hash_of(p, n));
    if (!s) { splint_id[i] = -1; strand[i] = '?'; }
    else { splint_id[i] = s->splint; strand[i] = s->strand == '-' ? '-' : '+'; ++n_ok; }
  }
  return n_ok;
}

// adapter_set of bin/preprocess.py:34,43: flags[s] = 1 when a counted row names splint s
extern "C" int c3_assign_seen(const c3_assign* a, uint8_t* flags, int64_t* rows_kept) {
  if (!a || !flags) return C3_E_ARG;
  memcpy(flags, a->seen.data(), a->seen.size());
  if (rows_kept) *rows_kept = a->rows_kept;
  return C3_E_OK;
}

// ---- PSL rows of the GPU splint finder (c3_scan_splints) written natively ------------------------------------------
// One 21-column row per assigned read of the group, appended to `path`: col 0 = equivalent perfect-match length m of the
// track maximum (match*m*(m+1)/2 = max, capped at the splint length), col 5 = 0, strand, read name, read length, query
// span, splint name / length -- the row psl_row() of c3poa_amd/preprocess.py states in Python.
extern "C" int c3_write_splint_psl(const c3_host_batch* b, const int32_t* table, const int16_t* splint_id, const char* strand,
                                   int n_splints, const char* const* splint_names, const int32_t* splint_lens, int match,
                                   const char* path, int64_t* rows_written) {
  if (!b || !table || !splint_id || !strand || n_splints <= 0 || !splint_names || !splint_lens || match <= 0 || !path) return C3_E_ARG;
  std::string out;
  out.reserve((size_t)b->n * 96);
  int64_t rows = 0;
  char tmp[256];
  for (int i = 0; i < b->n; ++i) {
    const int s = splint_id[i];
    if (s < 0 || s >= n_splints) continue;
    const int rc = strand[i] == '-' ? 1 : 0;
    const int32_t* e = table + (((size_t)i * n_splints + s) * 2 + rc) * 4;
    const long long L = b->off[i + 1] - b->off[i];
    const int S = splint_lens[s];
    const long long score = e[0] > 0 ? e[0] : 0;
    long long m = (long long)((std::sqrt(1.0 + 8.0 * (double)score / (double)match) - 1.0) / 2.0);
    if (m > S) m = S;
    long long q0 = e[1]; if (q0 < 0) q0 = 0; if (q0 > L) q0 = L;
    long long q1 = q0 + S; if (q1 > L) q1 = L;
    int k = snprintf(tmp, sizeof(tmp), "%lld\t%lld\t0\t0\t0\t0\t0\t0\t%c\t", m, (long long)S - m, rc ? '-' : '+');
    out.append(tmp, (size_t)k);
    out.append(b->names + b->name_off[i], (size_t)(b->name_off[i + 1] - b->name_off[i]));
    k = snprintf(tmp, sizeof(tmp), "\t%lld\t%lld\t%lld\t", L, q0, q1);
    out.append(tmp, (size_t)k);
    out.append(splint_names[s]);
    k = snprintf(tmp, sizeof(tmp), "\t%d\t0\t%d\t1\t%d,\t%lld,\t0,\n", S, S, S, q0);
    out.append(tmp, (size_t)k);
    ++rows;
  }
  if (!out.empty()) {
    FILE* f = fopen(path, "ab");
    if (!f) return C3_E_ARG;
    size_t w = fwrite(out.data(), 1, out.size(), f);
    if (fclose(f) != 0 || w != out.size()) return C3_E_ARG;
  }
  if (rows_written) *rows_written = rows;
  return C3_E_OK;
}
