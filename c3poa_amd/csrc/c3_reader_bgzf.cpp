// c3_reader_bgzf.cpp -- the BGZF input stream of the reader: members located by their headers, a stretch of them loaded beside
// the one being parsed, in one of three modes (c3_reader_bgzf.h).  Host code only.
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstring>

#include "c3_reader_bgzf.h"

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

namespace {

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

// a plain gzip file (c3_reader_gunzip_on_device): the next stretch of its stream, parsed on the device or brought to dec
bool gunzip_next_stretch(Bgzf* bz, BgzfStretch* b) {
  b->dend = 0; b->on_dev = false;
  if (bz->eof) return false;
  int eof = 0; int64_t bytes = 0;
  if (bz->parse_on) {
    const int rc = c3_gunzip_stream_next_parse(bz->gs, (int)(b - bz->st), bz->carry_from, bz->carry_len, &eof, &bytes, &b->fq);
    if (rc != C3_E_OK) { bz->why = c3_last_error(nullptr); bz->bad = true; return false; }
    if (eof) bz->eof = true;
    if (bytes == 0 && bz->carry_len == 0) return false;          // (an empty file, or nothing behind the last stretch)
    b->on_dev = true; b->next_rec = 0;
    ++bz->n_dev;
    return true;
  }
  if (bz->parse_req) ++bz->n_host;
  const char* text = nullptr;
  const int rc = c3_gunzip_stream_next(bz->gs, &text, &bytes, &eof);
  if (rc != C3_E_OK) { bz->why = c3_last_error(nullptr); bz->bad = true; return false; }
  if (eof) bz->eof = true;
  if (bytes == 0) return false;
  b->dec.assign(text, text + bytes);
  b->dend = (size_t)bytes;
  return true;
}

// next stretch of the file: up to `max_members` members read, located by their headers, inflated by b->threads threads
bool bgzf_next_stretch(Bgzf* bz, BgzfStretch* b, size_t max_members = 512) {
  if (bz->gs) return gunzip_next_stretch(bz, b);
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

// the turn to the next stretch, timed as waiting (c3_reader_inflate_wait): the stretch loaded beside the current one becomes the
// current one (the file's first is loaded here), `settle` takes note of it, and unless it objects the one after it starts
// loading on a thread of its own.  false: nothing more was loaded (end of file, or b->bad)
template <class F> bool bgzf_turn(Bgzf* b, F&& settle) {
  struct Wait { Bgzf* b; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
                ~Wait() { b->wait_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); } } wait{b};
  bool loaded;
  if (b->pre_on) { b->pre.join(); b->pre_on = false; loaded = b->pre_ok; if (loaded) b->cur ^= 1; }
  else loaded = !b->bad && bgzf_next_stretch(b, &b->st[b->cur]);
  if (b->bad || !loaded) return false;
  if (settle(b->st[b->cur]) && !b->eof) { BgzfStretch* nx = &b->st[b->cur ^ 1]; b->pre_on = true; b->pre = std::thread([b, nx]() { b->pre_ok = bgzf_next_stretch(b, nx); }); }
  return true;
}

}  // namespace

// bytes of the inflated file, in order.  While the parser works through one stretch the next one is read and inflated on a
// thread of its own (which fans out to b->threads inflaters): the reader thread only waits when inflating is the slower side
long bgzf_read(Bgzf* b, char* dst, size_t room) {
  if (b->dpos == b->st[b->cur].dend) {
    b->dpos = 0;
    if (!bgzf_turn(b, [](BgzfStretch&) { return true; })) { b->st[b->cur].dend = 0; return b->bad ? -1 : 0; }
  }
  BgzfStretch& c = b->st[b->cur];
  const size_t k = std::min(room, c.dend - b->dpos);
  memcpy(dst, c.dec.data() + b->dpos, k);
  b->dpos += k;
  return (long)k;
}

// the same turn for stretches parsed on the device: what the next load needs to know of the new current stretch is noted
// before that load starts
bool dev_advance(Bgzf* b) {
  if (!b->pre_on && !b->bad) b->carry_from = b->carry_len = 0;  // (the file's first stretch)
  return bgzf_turn(b, [b](BgzfStretch& c) {
    if (c.fq.info.departed) b->parse_on = false;                // from here on the host parser (the next load already goes its way)
    b->carry_from = c.fq.info.consumed; b->carry_len = c.fq.text_bytes - c.fq.info.consumed;
    if (b->bam) {
      c.base_off = b->dev_base; b->dev_base += c.fq.info.consumed;
      if (c.fq.header_bytes > 0) b->bam_at_start = false;
      if (c.fq.info.departed) return false;                     // a departure is the reader's error: nothing more is loaded
    }
    return true;
  });
}
