// c3_reader.cpp -- native host input in front of the hot path: streaming FASTA / FASTQ (.gz, BGZF) / BAM
// reader that fills structure-of-arrays host batches in page-locked memory (so c3_batch_upload copies them by DMA), or
// leaves the bases of a group on the device.  A group is built by one Group object that three record sources fill: records of
// the device stretches, BAM records, text lines.  Host code only: no kernels here, nothing here touches the oracle.
//
//   c3_reader_*      replaces mm.fastx_read(args.reads, read_comment=False)   (C3POa.py:201,239; kseq.h semantics)
#include <zlib.h>

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/c3poa.h"
#include "c3_checks.h"
#include "c3_bam.h"
#include "c3_hostbuf.h"
#include "c3_reader_bgzf.h"

namespace {

struct BatchSet {
  HostBuf names, seqs, quals;
  std::vector<int64_t> name_off, off;
  size_t n_names = 0, n_bases = 0;
  bool on_dev = false;                      // the group it holds is a device group: its bases lie in the reader's device set (c3_reader_stage_on_device)
};

}  // namespace

struct c3_reader {
  FILE* fp = nullptr; gzFile gz = nullptr; Bgzf* bz = nullptr;
  // c3_reader_open_inflate on plain gzip: the device it was given (c3_reader_gunzip_on_device hands it to bz) and the path
  c3_bgzf* gz_dev = nullptr; std::string path;
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

bool refill(c3_reader* r) {
  if (r->eof) return false;
  if (r->beg > 0) { memmove(r->buf.data(), r->buf.data() + r->beg, r->end - r->beg); r->end -= r->beg; r->buf_off += (int64_t)r->beg; r->beg = 0; }
  if (r->end == r->buf.size()) r->buf.resize(r->buf.size() * 2);
  size_t room = r->buf.size() - r->end;
  long got = r->bz ? bgzf_read(r->bz, r->buf.data() + r->end, room)
           : r->gz ? (long)gzread(r->gz, r->buf.data() + r->end, (unsigned)std::min<size_t>(room, 1u << 30))
                   : (long)fread(r->buf.data() + r->end, 1, room, r->fp);
  if (got < 0 && r->bz) r->err = r->bz->gs ? r->bz->why : "BGZF input: a member is damaged (size, inflate or CRC)" + (r->bz->why.empty() ? std::string() : ": " + r->bz->why);
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
  r->path = path;
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
  } else if (r->gz) r->gz_dev = z;                              // plain gzip: read as c3_reader_open reads it unless c3_reader_gunzip_on_device follows
  else c3_bgzf_destroy(z);                                      // plain text
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
  if (r->gz_dev) c3_bgzf_destroy(r->gz_dev);
  if (r->gz) gzclose(r->gz);
  if (r->fp) fclose(r->fp);
  if (r->bz) { if (r->bz->pre_on) r->bz->pre.join(); if (r->bz->fp) fclose(r->bz->fp); if (r->bz->gs) c3_gunzip_stream_close(r->bz->gs); if (r->bz->dev) c3_bgzf_destroy(r->bz->dev); delete r->bz; }
  delete r;
}

// names_only != 0: sequences and qualities are parsed (lengths, offsets and the short-read count stay exact) but not
// stored -- the first pass of C3POa.py:200-207 only needs names
extern "C" void c3_reader_names_only(c3_reader* r, int names_only) { if (r) r->names_only = names_only != 0; }

extern "C" int c3_reader_parse_on_device(c3_reader* r, int on) {
  if (!r) return C3_E_ARG;
  if (!r->bz || !r->bz->dev) { r->err = "c3_reader_parse_on_device: not a BGZF file opened by c3_reader_open_inflate, nor a plain gzip file with c3_reader_gunzip_on_device"; return C3_E_STATE; }
  if (r->started) { r->err = "c3_reader_parse_on_device: after the first c3_reader_next"; return C3_E_STATE; }
  r->bz->parse_req = r->bz->parse_on = r->bz->dev_active = on != 0;
  return C3_E_OK;
}

// a plain gzip file opened by c3_reader_open_inflate is inflated by the k_gunzip kernels on that device instead of gzread: the
// reader becomes one of the BGZF kind (stretch loop, prefetch thread, device parser and device groups) whose stretches are what
// the gzip stream inflates next
extern "C" int c3_reader_gunzip_on_device(c3_reader* r, int on) {
  if (!r) return C3_E_ARG;
  if (r->bz && r->bz->gs) {
    if (on) return C3_E_OK;
    r->err = "c3_reader_gunzip_on_device: cannot be taken back"; return C3_E_STATE;
  }
  if (!r->gz || !r->gz_dev) { r->err = "c3_reader_gunzip_on_device: not a plain gzip file opened by c3_reader_open_inflate"; return C3_E_STATE; }
  if (r->started) { r->err = "c3_reader_gunzip_on_device: after the first c3_reader_next"; return C3_E_STATE; }
  if (!on) return C3_E_OK;
  c3_gunzip_stream* gs = nullptr;
  const int rc = c3_gunzip_stream_open(r->gz_dev, r->path.c_str(), &gs);
  if (rc != C3_E_OK) { r->err = c3_last_error(nullptr); return rc; }
  gzclose(r->gz); r->gz = nullptr;
  r->bz = new Bgzf(); r->bz->gs = gs; r->bz->dev = r->gz_dev; r->gz_dev = nullptr;
  return C3_E_OK;
}

extern "C" int c3_reader_gunzip_stats(const c3_reader* r, int64_t* v, int n) {
  if (!r || !v || n < 0) return C3_E_ARG;
  c3_gunzip_stream_stats(r->bz ? r->bz->gs : nullptr, v, n);
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

// First kept record (sl bases) of a reader's very first group: the bytes of max_reads records of this length, for ONE page-locked
// allocation instead of a dozen grow-and-copy steps (page-locking is slow and serialised by the driver).  What the reader can
// still deliver, which caps it, differs between the three sources and stays with each (Group::size takes it as `deliver`).
size_t first_group_estimate(int max_reads, int64_t max_bases, size_t sl) {
  size_t want = (size_t)max_reads * (sl + sl / 4) + 4096;
  if (max_bases > 0) want = std::min(want, (size_t)max_bases + sl + 4096);
  return std::min(want, (size_t)2 << 30);
}

// One group of reads being built in buffer set `set`: the group rule, the running counts, where its bases go and how their room
// is sized.  The three sources below fill it; nothing else in this file states any of these.
struct Group {
  // where the bases go: the page-locked host set; the device set of the same number (c3_reader_stage_on_device); or that
  // device set for as long as the device source has its turn -- its first record makes the group a device group, which ends in
  // front of a departure or at the end of the device's records, and none leaves an ordinary host group (settle)
  enum Dest { HOST, DEVICE, UNDECIDED };
  c3_reader* const r; BatchSet& s; const int set;
  const int max_reads; const int64_t max_bases; const int min_len;
  int n = 0; size_t nn = 0, nb = 0; int64_t n_short = 0;
  Dest dest = HOST;
  bool hint_due = false;          // the host set of a staging reader is sized like a later set only once the text does hold a record

  Group(c3_reader* r_, int set_, int max_reads_, int64_t max_bases_, int min_len_)
      : r(r_), s(r_->sets[(size_t)set_]), set(set_), max_reads(max_reads_), max_bases(max_bases_), min_len(min_len_) {
    s.name_off.assign(1, 0); s.off.assign(1, 0);
    s.on_dev = false;
  }
  bool open() const { return n < max_reads && (max_bases <= 0 || (int64_t)nb < max_bases); }
  bool keeps(int64_t len) const { return len >= (int64_t)min_len; }
  void push(size_t name_len, size_t len) {
    if (dest == UNDECIDED) dest = DEVICE;
    nn += name_len; nb += len; ++n;
    s.name_off.push_back((int64_t)nn); s.off.push_back((int64_t)nb);
  }
  // `want` bytes per array of set `o` (this group's or another one of the reader), its first `keep` kept
  int reserve(BatchSet& o, size_t want, size_t keep) {
    if (dest == HOST) return o.seqs.reserve(want, keep) && o.quals.reserve(want, keep) ? C3_E_OK : C3_E_NOMEM;
    if (c3_bgzf_set_reserve(r->bz->dev, (int)(&o - r->sets.data()), (int64_t)want, (int64_t)keep) == C3_E_OK) return C3_E_OK;
    r->err = c3_last_error(nullptr);
    return C3_E_NOMEM;
  }
  // later sets are allocated once, with the size the previous groups needed (growth by copying only for the first)
  size_t hint() const { return r->hint_bases + r->hint_bases / 8 + 4096; }
  // at entry: while the device parser hands out records a staging reader builds the group in the device set; the hint goes to
  // the side the group starts on, or waits for the first header line of the text (fill_from_text)
  int begin() {
    const bool staging = r->bz && r->bz->stage_on && !r->names_only;
    if (staging && r->bz->dev_active) dest = UNDECIDED;
    if (r->names_only || !r->hint_bases) return C3_E_OK;
    if (staging && dest == HOST) { hint_due = true; return C3_E_OK; }
    return reserve(s, hint(), 0);
  }
  // the device source has had its turn and left no record: the call goes on as a host group, in the page-locked set
  void settle() { if (dest == UNDECIDED) { dest = HOST; hint_due = r->hint_bases != 0; } }
  int size_deferred() { if (!hint_due) return C3_E_OK; hint_due = false; return reserve(s, hint(), 0); }
  // no record kept yet (`pending` counted but still to be stored) in a reader that has not sized a group before
  bool first(int64_t pending = 0) const { return n == pending && !r->hint_bases && !r->names_only; }
  // Room for the bases: `need` bytes per array, the first `keep` valid.  The first kept record (sl bases) of the very first group
  // asks for first_group_estimate, never more than the `deliver` bytes its source can still yield, and for the other buffer sets
  // of the reader right away, as many bytes each: a page-lock issued later, while the GPU is busy, stalls the running kernels for
  // its whole duration (some 50 ms per 400 MiB).  Only as many sets as `deliver` could fill are reserved now (a 100-read input
  // used to pin ten buffers of max_reads reads each); the rest grow lazily if ever needed.
  int size(size_t need, size_t keep, size_t sl, size_t deliver, int64_t pending = 0) {
    if (r->names_only) return C3_E_OK;
    size_t want = need;
    if (first(pending)) {
      want = std::max(want, std::min(first_group_estimate(max_reads, max_bases, sl), deliver));
      size_t left = deliver > want ? deliver - want : 0;
      for (BatchSet& o : r->sets) if (&o != &s) {
        if (left == 0) break;
        const size_t w2 = std::min(want, left + 4096);
        if (const int rc = reserve(o, w2, 0)) return rc;
        left -= std::min(left, w2);
      }
    }
    return reserve(s, want, keep);
  }
  void finish(c3_host_batch* out) {
    s.n_names = nn; s.n_bases = nb;
    r->hint_bases = std::max(r->hint_bases, nb);
    out->n = n; out->n_short = n_short;
    out->names = s.names.p; out->name_off = s.name_off.data();
    out->seqs = s.seqs.p; out->quals = s.quals.p; out->off = s.off.data();
    if (dest == DEVICE) { s.on_dev = true; out->seqs = out->quals = nullptr; ++r->bz->grp_dev; }
    else if (r->bz && r->bz->stage_on && n > 0) { ++r->bz->grp_host; r->bz->host_bytes += 2 * (int64_t)nb; }
  }
};

// what a compressed file can still deliver to a first group (compressed size: a generous bound)
size_t deliver_compressed(const c3_reader* r, size_t sl) { return r->file_bytes ? r->file_bytes * 16 + sl + 4096 : (size_t)-1; }

// Source 1, c3_reader_parse_on_device: records of the device stretches, in runs that enter the group with one copy per array
// from the device straight to the set's fill offsets (or, staging, device to device).  Returns with the group closed, at the
// end of the file, or with the rest of the text handed to the host parser (a departure).
int fill_from_device(Group& g) {
  c3_reader* r = g.r; Bgzf* b = r->bz; BatchSet& s = g.s;
  const bool stage = g.dest != Group::HOST;                       // the bases stay on the device, in the set of the same number
  while (g.open()) {
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
    if (!g.keeps(off[j + 1] - off[j])) { ++g.n_short; ++r->n_records; ++b->rec_dev; c->next_rec = j + 1; continue; }
    // a run of records that all enter the group: it ends at the stretch's end, at a short record or when the group closes
    const int64_t j0 = j, sl0 = off[j + 1] - off[j];
    const size_t nn0 = g.nn, nb0 = g.nb;
    for (; j < nk && g.open() && g.keeps(off[j + 1] - off[j]); ++j) g.push((size_t)(noff[j + 1] - noff[j]), (size_t)(off[j + 1] - off[j]));
    if (!s.names.reserve(g.nn + 16, nn0)) return C3_E_NOMEM;
    if (const int rc = g.size(g.nb + 16, nb0, (size_t)sl0, deliver_compressed(r, (size_t)sl0), j - j0)) return rc;
    const int rc = stage ? c3_bgzf_stretch_stage(b->dev, b->cur, j0, j, s.names.p + nn0, g.set, (int64_t)nb0)
                         : c3_bgzf_stretch_fetch(b->dev, b->cur, j0, j, s.names.p + nn0, r->names_only ? nullptr : s.seqs.p + nb0, r->names_only ? nullptr : s.quals.p + nb0);
    if (rc != C3_E_OK) { b->why = c3_last_error(nullptr); b->bad = true; b->dev_active = false; break; }
    r->n_records += j - j0; b->rec_dev += j - j0;
    c->next_rec = j;
  }
  return C3_E_OK;
}

// Source 2, a .bam file: records by the rule of c3_bam.h (what c3_bam_parse_host applies) over the bytes bgzf_read yields
int fill_from_bam(Group& g) {
  c3_reader* r = g.r; BatchSet& s = g.s;
  if (!r->bz) return fail(r, "BAM input: not a BGZF file");
  while (g.open()) {
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
      if (r->bz->bad || (r->bam_hdr && r->beg == r->end)) break;     // a damaged member (the caller reports it), or the end of the file
      return bam_fail(r, C3_BAM_TRUNCATED, r->bam_hdr ? at : 0);
    }
    if (st != C3_BAM_OK) return bam_fail(r, st, r->bam_hdr ? at : 0);
    r->beg = (size_t)rec.next;
    ++r->n_records;
    const size_t sl = rec.l_seq;
    if (!g.keeps((int64_t)sl)) { ++g.n_short; continue; }
    if (!s.names.reserve(g.nn + rec.name_len + 16, g.nn)) return C3_E_NOMEM;
    memcpy(s.names.p + g.nn, d + rec.name, rec.name_len);
    if (const int rc = g.size(g.nb + sl + 16, g.nb, sl, deliver_compressed(r, sl))) return rc;
    if (!r->names_only) {
      char* sq = s.seqs.p + g.nb; char* ql = s.quals.p + g.nb;
      for (size_t i = 0; i < sl; ++i) { sq[i] = (char)c3_bam_base_at(d + rec.seq, (int64_t)i); ql[i] = (char)c3_bam_qual(d[rec.qual + i]); }
    }
    g.push(rec.name_len, sl);
  }
  return C3_E_OK;
}

// Source 3, FASTA / FASTQ text (kseq.h semantics).  The bytes of a record are written before its length is known: a short one
// is dropped by not pushing it, and the next record overwrites it.
int fill_from_text(Group& g) {
  c3_reader* r = g.r; BatchSet& s = g.s;
  const char* p; size_t l;
  while (g.open()) {
    if (!next_line(r, &p, &l)) break;
    if (l == 0) continue;
    if (p[0] != '>' && p[0] != '@') return fail(r, "not FASTA/FASTQ: record does not start with '>' or '@'");
    if (const int rc = g.size_deferred()) return rc;
    if (r->range_end >= 0 && r->buf_off + (int64_t)(p - r->buf.data()) >= r->range_end) { r->eof = true; r->beg = r->end; break; }   // next range's record
    // name = header up to the first blank (read_comment=False)
    size_t nl = 1; while (nl < l && p[nl] != ' ' && p[nl] != '\t') ++nl;
    if (!s.names.reserve(g.nn + nl, g.nn)) return C3_E_NOMEM;
    memcpy(s.names.p + g.nn, p + 1, nl - 1);
    const size_t name_len = nl - 1;
    // sequence lines until a line that starts with '>', '@' or '+' (kseq.h)
    const size_t sb = g.nb; size_t sl = 0; bool plus = false;
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
    if (!g.keeps((int64_t)sl)) { ++g.n_short; continue; }            // dropped: buffers are simply overwritten
    if (sl > 0 && g.first()) {
      // the record is in place already (keep = sb + sl).  This reader can still deliver no more than half of the bytes left in
      // its file / byte range as sequence bytes (the other half are qualities)
      size_t deliver = (size_t)-1;
      if (!r->gz && !r->bz && r->file_bytes) {
        const int64_t stop = r->range_end >= 0 ? std::min<int64_t>(r->range_end + (int64_t)(4 * sl + 4096), (int64_t)r->file_bytes) : (int64_t)r->file_bytes;
        const int64_t here = r->buf_off + (int64_t)r->beg;
        deliver = (size_t)std::max<int64_t>(0, stop - here) / 2 + sb + sl + 4096;
      } else deliver = deliver_compressed(r, sb + sl);
      if (const int rc = g.size(0, sb + sl, sl, deliver)) return rc;
    }
    g.push(name_len, sl);
  }
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
  Group g(r, set, max_reads, max_bases, min_len);                 // (resets the set)
  int rc = g.begin();
  if (rc != C3_E_OK) return rc;
  r->started = true;
  if (r->bz && r->bz->dev_active) rc = fill_from_device(g);       // c3_reader_parse_on_device: the device parser fills the group ...
  if (rc == C3_E_OK && g.dest != Group::DEVICE) {                 // ... and after a departure the host goes on with the same group
    g.settle();
    rc = r->bam ? fill_from_bam(g) : fill_from_text(g);
  }
  if (rc != C3_E_OK) return rc;
  if (r->bz && r->bz->bad && r->bz->gs) { r->err = r->bz->why; return C3_E_DATA; }      // (c3_gunzip's text: member, offset, reason)
  if (r->bz && r->bz->bad) return fail(r, "BGZF input: a member is damaged (header, size, inflate or CRC)");      // never a silently short file
  g.finish(out);
  return C3_E_OK;
}
