// k_poa_pair.hip -- the alignment of subread 1 against the bare chain of subread 0, ahead of k_poa.
//
// For subread 1 the POA graph is the chain of subread 0: position idx of the topological order holds node idx + 1, every row's
// one predecessor is the row above, the row's base is base idx - 1 of subread 0 and its nominal column is Q1 - (Q0 - idx).
// Nothing poa_align<false, true, false> looks up for that alignment needs the graph, so this kernel computes it from the
// packed read alone -- no descriptor sweep, no descriptor broadcasts, no row records from lane 0, no far / capacity / WIDE
// tests, no ring stores of rows nobody reads back -- and leaves, per read, vq[q] (the node aligned to base q, 0xffff = insertion),
// the counted cells and a done flag.  k_poa then skips poa_align at s == 1 for flagged reads and feeds vq to poa_fuse.
//
// ONE WAVE PER READ, persistent over k_poa's cost-sorted work list, abPOA's default scoring and the NARROW geometry only.
// Cells, bases, guards, tie-order tags and direction bytes are those of k_poa's fast, two-column and one-chunk near rows (the row
// code is a copy, not shared: k_poa's register budget is its own).  A read this kernel cannot take exactly -- Q1 > 1792, a row
// wider than 128 columns or empty, a guard trip, a failed end cell, scratch of the slot too small -- is DECLINED: its flag stays
// 0 and k_poa aligns it as before.  Scratch: the slot's k_poa arenas (idle while this kernel runs on the same stream).
#include "c3_dev.h"
#include "c3_args.h"
#include "c3_launch.h"

#define WSYNC() __syncthreads()
#define PADL 3
#define PW 128
#define PWT (PADL + PW + 3)
#define PQW 112                       // packed query words of subread 1 that fit the LDS table: 1792 bases
#define DSTRIDE 128                   // direction bytes of a row: fixed stride, byte k = column band begin + k
// 16-bit cells: (score - row base) * 8 + BIAS16, as in k_poa.hip
#define S3(x) ((x) * 8)
#define BIAS16 32768
#define NEG16 6000
#define NEG2_16 2000
#define FLOOR16 5000
#define ZHI16 12000
#define GLO16 14400
#define ZLO16 13200
#define RB_LO16 (BIAS16 - 400 * 8)
#define RB_HI16 (BIAS16 + 3000 * 8)
__device__ __forceinline__ int maxu16(int a, int b) { int d; asm volatile("v_max_u16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ int minu16(int a, int b) { int d; asm volatile("v_min_u16 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
// lane in mask m ? t : f.  The mask of a row's active lanes is made once per row on the scalar unit (no compare in the row)
__device__ __forceinline__ int selm(unsigned long long m, int t, int f) { int d; asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(d) : "v"(f), "v"(t), "s"(m)); return d; }

// Query bytes: base q of subread 1 as code * 8 in qb[QOFF + q], so column j's base (q = j - 1) is ONE byte read at beg + lane + a
// constant and the byte is the bit offset of the row's substitution addend in a 4-byte table (v_bfe_i32).  qb[QOFF - 1] repeats
// base 0: column 0's diagonal candidate is built on the left pad of the row above and loses either way, and with base 0 there it
// keeps the very value it had when the column index was clamped.  The QBACK bytes behind the last word are only ever read by
// idle lanes (an active column is <= Q1), whose cells are replaced before use.
#define QOFF 16
#define QBACK 128
#define QBN (QOFF + PQW * 16 + QBACK)
// two ring rows (the row above a two-column / near row, and the row being written); the traceback's direction windows reuse them
struct alignas(16) PairLds { union { unsigned short ring[3][2][PWT]; uint8_t win[64 * 32]; }; uint8_t qb[QBN]; };
__shared__ PairLds L;
// the four 2-bit codes of a byte as four bytes of code * 8
__device__ __forceinline__ unsigned pair_spread8(unsigned x) {
  return ((x & 3u) | ((x & 0xcu) << 6) | ((x & 0x30u) << 12) | ((x & 0xc0u) << 18)) << 3;
}

// returns the counted cells (> 0), or -1: declined
__device__ int pair_align(const PoaPairArgs& a, const uint32_t* pk, int qb0, int Q0, int qb1, int Q1, uint8_t* D, int* rowrec, uint16_t* vq, int lane) {
  constexpr int mt8 = S3(5), mm8 = S3(-4), e1_8 = S3(2), e2_8 = S3(1), o1_8 = S3(4), o2_8 = S3(24), oe1_8 = o1_8 + e1_8, oe2_8 = o2_8 + e2_8;
  // (vq holds the node row + 1 in 16 bits, 0xffff = insertion)
  if (Q0 < 1 || Q1 < 1 || Q1 > PQW * 16 || Q0 + 1 >= 0xffff || Q0 + 2 > a.Ncap || (long long)(Q0 + 1) * DSTRIDE + 64 > a.dbytes) return -1;
  const int rb_span = a.rb_span > 0 ? a.rb_span : RB_HI16 - RB_LO16;
  const int w = wave_first(a.p.band_b + (int)(a.p.band_f * (double)Q1));
  const int le1_8 = e1_8 * lane, le2_8 = e2_8 * lane, lo1_8 = le1_8 + o1_8, lo2_8 = le2_8 + o2_8, lane4 = lane * 4;
  unsigned short (*LH)[PWT] = L.ring[0]; unsigned short (*LE1)[PWT] = L.ring[1]; unsigned short (*LE2)[PWT] = L.ring[2];
  WSYNC();                                                         // (the windows of the read before are done with)
  for (int i = lane; i < PQW && 16 * i < Q1; i += 64) {
    const long long b0 = (long long)qb1 + 16 * i;
    const unsigned w0 = pk[b0 >> 4], w1 = pk[(b0 >> 4) + 1];
    const unsigned x = __builtin_amdgcn_alignbit(w1, w0, (unsigned)(b0 & 15) * 2);
    const uint4 o = make_uint4(pair_spread8(x & 0xffu), pair_spread8((x >> 8) & 0xffu), pair_spread8((x >> 16) & 0xffu), pair_spread8(x >> 24));
    *(uint4*)&L.qb[QOFF + 16 * i] = o;
    if (i == 0) L.qb[QOFF - 1] = (uint8_t)o.x;
  }
  if (lane < QBACK / 4) *(unsigned*)&L.qb[QOFF + 16 * ((Q1 + 15) >> 4) + 4 * lane] = 0;
  { unsigned* r32 = (unsigned*)&L.ring[0][0][0]; for (int i = lane; i < 3 * 2 * PWT / 2; i += 64) r32[i] = NEG16 | (NEG16 << 16); }
  WSYNC();
  // ---- row 0 (the source): H[0][j] = the better of the two gap openings from column 0, as the general row leaves it
  int u_beg = 0, u_end = min(Q1, max(Q1 - Q0, 0) + w), u_left = 0, u_right = 0, u_b8 = 0;
  if (u_end + 1 > PW) return -1;
  if (u_end < u_beg) { u_left = INT32_MAX / 2 - 1; u_right = -1; }  // an empty source row (w < 0) bounds row 1 by qr alone
  int ncell = u_end + 1, u_cap = min(Q1, u_end + 1);
  int pH = NEG16, pE1 = NEG16, pE2 = NEG16;
#pragma unroll
  for (int ch = 0; ch < 2; ++ch) {
    const int j = 64 * ch + lane;
    const int sc = j == 0 ? 0 : max(-(4 + 2 * j), -(24 + j));
    const int h = j <= u_end ? BIAS16 + S3(sc) : NEG16;
    const unsigned d = j == 0 ? 40u : (8u | ((j <= 20 ? 1u : 0u) << 4) | (j >= 2 ? 192u : 0u));
    LH[0][PADL + j] = (unsigned short)h;
    if (j <= u_end) D[j] = (uint8_t)d;
    if (ch == 0) pH = h;
  }
  // the row above is in pH / pE1 / pE2 (lane = band column): pvk = 64 - its width, the lanes it leaves idle; else pvk < 0.
  // (Numbers, not flags: a carried flag is a 64-bit lane mask to the compiler, and every test of it three scalar instructions)
  int pvk = 63 - u_end;
  int in_ring = 1, rs = 0;                                         // ... is in ring slot rs
  int Q0run = Q0;                                                  // a declined read ends both loops through their one exit
  int gacc = 0xffff, punt = 0;
  // The uniform state of a row (u_*, qr, the band, the masks of its active lanes) lives on the scalar unit only: no vector
  // instruction of the band arithmetic.  The lanes see the band through three SGPR operands a row: beg (query byte), the
  // substitution table and the mask
  const int vneg = NEG16, vneg2 = NEG2_16;
  const int qrel = Q1 - Q0, cells_lim = a.cells_cap - PW;
  int li0 = 1;                                                     // block 0 starts at row 1 (a carried constant, not a compare turned into a number)
  unsigned voff = DSTRIDE + (unsigned)lane;                        // direction byte of the lane in row 1: rows follow at DSTRIDE
  for (int ib = 0; ib <= Q0run; ib += 64) {
    const int ridx = ib + lane;
    // the row's substitution addends (tag 2 included), byte c = base code c of the query: mismatch, but the row's own base
    const int vbv = (ridx >= 1 && ridx <= Q0) ? (int)(0x01010101u * (unsigned)((mm8 + 2) & 0xff) ^ ((unsigned)((mm8 + 2) ^ (mt8 + 2)) & 0xffu) << (8 * c3_code_at(pk, (int64_t)qb0 + ridx - 1))) : 0;
    int recv = (ib == 0 && lane == 0) ? ((u_end + 1) << 16) : 0;  // row records: band begin | width << 16, lane = row of the block
    const int cnt = min(64, Q0 + 1 - ib);
    for (int li = li0; li < cnt; ++li) {
      const int qr = qrel + ib + li;
      const int tab = __builtin_amdgcn_readlane(vbv, li);
      // band from the row above (C3_BAND_OF_ROW_ABOVE of k_poa; the row above is never empty: an empty row declines below)
      // (u_beg >= 0 and u_cap = min(Q1, u_end + 1) make each bound ONE max / min: a three-operand form exists on the vector unit only)
      const int beg = max(min(u_left + 1, qr) - w, u_beg);
      const int end = min(max(u_right + 1, qr) + w, u_cap);
      const int wd = end - beg + 1, sh = beg - u_beg;
      u_beg = beg; u_end = end; u_cap = min(Q1, end + 1);          // (the row above's are done with: sh and pvk carry what the row needs)
      // declined: wd < 1, wd > PW or ncell + PW > cells_cap -- one sign test
      if (((wd - 1) | (PW - wd) | (cells_lim - ncell)) < 0) { Q0run = -1; li = 64; gacc = 0; continue; }   // (nothing carried is read again)
      int left, right, nb8 = u_b8;
      if (wd <= 64) {
        // ---- one column per lane: the row above from registers (lane permutes) or from its ring slot (clamped offsets; pads
        // and idle cells hold NEG16)
        const unsigned long long am = ~0ull >> (64 - wd);            // lanes below wd
        const int q8 = L.qb[QOFF - 1 + beg + lane];
        int hd, hp, e1p, e2p;
        // registers valid, wd + sh <= 64, and lane 0's diagonal permute wraps into an idle lane: sh >= 1 or the row above left one
        if (min(sh | pvk, 65 - wd - sh) > 0) {
          const int a_p = lane4 + sh * 4, a_d = a_p - 4;
          hd = __builtin_amdgcn_ds_bpermute(a_d, pH); hp = __builtin_amdgcn_ds_bpermute(a_p, pH);
          e1p = __builtin_amdgcn_ds_bpermute(a_p, pE1); e2p = __builtin_amdgcn_ds_bpermute(a_p, pE2);
        } else {
          if (in_ring == 0) {
            rs ^= 1;
            LH[rs][PADL + lane] = (unsigned short)pH; LE1[rs][PADL + lane] = (unsigned short)pE1; LE2[rs][PADL + lane] = (unsigned short)pE2;
            LH[rs][PADL + 64 + lane] = NEG16; LE1[rs][PADL + 64 + lane] = NEG16; LE2[rs][PADL + 64 + lane] = NEG16;
          }
          const int ix = PADL + min(max(sh + lane, -2), PW + 1);
          hd = LH[rs][ix - 1]; hp = LH[rs][ix]; e1p = LE1[rs][ix]; e2p = LE2[rs][ix];
        }
        const int M = hd + __builtin_amdgcn_sbfe(tab, (unsigned)q8, 8u);         // Ht source in bits 0-1: M 2, E1 1, E2 0
        const int E1t = maxu16(hp - (oe1_8 - 1), e1p - e1_8);                  // bit 0 set: opened (open wins ties)
        const int E2t = maxu16(hp - (oe2_8 - 2), e2p - e2_8);                  // bit 1 set: opened
        const int E1c = E1t & ~7, E2c = E2t & ~7;
        const int k2 = maxu16(maxu16(M, E1c + 1), E2c);
        const int ht = k2 & ~7;
        const int htm = selm(am, ht, vneg2);
        int s1 = htm + le1_8, s2 = htm + le2_8, s3 = htm;
        wave_scan_max3(s1, s2, s3);
        const int px1 = wave_shr1(s1, NEG2_16), px2 = wave_shr1(s2, NEG2_16);
        const int htl = wave_shr1(htm, NEG16);
        const int f1 = px1 - lo1_8, f2 = px2 - lo2_8;
        const int k3 = maxu16(maxu16(ht + 2, f1 + 1), f2);                     // H source in bits 0-1: Ht 2, F1 1, F2 0
        const int h = k3 & ~7;
        // (the tags of E1t and E2t are bit 0 and bit 1, the other one clear in each: one and takes both)
        unsigned d = ((unsigned)(E1t | E2t) & 3u) | (((unsigned)k2 & 3u) << 2) | (((unsigned)k3 & 3u) << 4);
        d |= (((unsigned)(htl - oe1_8 - f1)) >> 25) & 64u;                      // f1 > its "open" candidate: extended
        d |= (((unsigned)(htl - oe2_8 - f2)) >> 24) & 128u;
        const int rb = __builtin_amdgcn_readlane(s3, 63);                       // row maximum (of Ht == of H)
        const unsigned long long mxm = __ballot(htm == rb);
        left = beg + __builtin_ctzll(mxm); right = beg + (63 - __builtin_clzll(mxm));
        pH = maxu16(selm(am, h, vneg), FLOOR16); pE1 = selm(am, E1c, vneg); pE2 = selm(am, E2c, vneg);
        if ((unsigned)(rb - RB_LO16) > (unsigned)rb_span) {                     // rare: the base follows the row maximum, saturating
          const int m1 = rb - BIAS16, fl1 = FLOOR16 + max(m1, 0);
          nb8 += m1; if (rb < GLO16) punt = 1;
          pH = selm(am, maxu16(h, fl1) - m1, vneg); pE1 = selm(am, maxu16(E1c, fl1) - m1, vneg); pE2 = selm(am, maxu16(E2c, fl1) - m1, vneg);
        }
        gacc = minu16(gacc, pH - (ZHI16 + 1));
        D[voff] = (uint8_t)d;                                                   // (unmasked: bytes past the band are never selected)
        pvk = 64 - wd; in_ring = 0;
      } else {
        // ---- two columns per lane (65-128 columns): the row above from its ring slot, this row into the other one
        if (in_ring == 0) {
          rs ^= 1;
          LH[rs][PADL + lane] = (unsigned short)pH; LE1[rs][PADL + lane] = (unsigned short)pE1; LE2[rs][PADL + lane] = (unsigned short)pE2;
          LH[rs][PADL + 64 + lane] = NEG16; LE1[rs][PADL + 64 + lane] = NEG16; LE2[rs][PADL + 64 + lane] = NEG16;
        }
        const int c0l = 2 * lane;
        const unsigned long long am0 = ~0ull >> (64 - ((wd + 1) >> 1)), am1 = ~0ull >> (64 - (wd >> 1));   // 2 lane (+ 1) < wd
        const uint8_t* const qp = &L.qb[QOFF - 1 + beg + c0l];
        const int q80 = qp[0], q81 = qp[1];
        const int rx = PADL + min(sh + c0l, PW);                                 // column j0 in the row above (active columns: [-1, its width])
        const int hd0 = LH[rs][rx - 1], hp0 = LH[rs][rx], hp1 = LH[rs][rx + 1];
        const int e1p0 = LE1[rs][rx], e1p1 = LE1[rs][rx + 1], e2p0 = LE2[rs][rx], e2p1 = LE2[rs][rx + 1];
        const int M0 = hd0 + __builtin_amdgcn_sbfe(tab, (unsigned)q80, 8u), M1 = hp0 + __builtin_amdgcn_sbfe(tab, (unsigned)q81, 8u);
        const int E1t0 = maxu16(hp0 - (oe1_8 - 1), e1p0 - e1_8), E1t1 = maxu16(hp1 - (oe1_8 - 1), e1p1 - e1_8);
        const int E2t0 = maxu16(hp0 - (oe2_8 - 2), e2p0 - e2_8), E2t1 = maxu16(hp1 - (oe2_8 - 2), e2p1 - e2_8);
        const int E1c0 = E1t0 & ~7, E2c0 = E2t0 & ~7, E1c1 = E1t1 & ~7, E2c1 = E2t1 & ~7;
        const int k20 = maxu16(maxu16(M0, E1c0 + 1), E2c0), k21 = maxu16(maxu16(M1, E1c1 + 1), E2c1);
        const int ht0 = k20 & ~7, ht1 = k21 & ~7;
        const int htm0 = selm(am0, ht0, vneg2), htm1 = selm(am1, ht1, vneg2);
        const int l1 = e1_8 * c0l, l2 = e2_8 * c0l;
        const int t10 = htm0 + l1, t20 = htm0 + l2;
        int s1 = max(t10, htm1 + l1 + e1_8), s2 = max(t20, htm1 + l2 + e2_8), s3 = max(htm0, htm1);
        wave_scan_max3(s1, s2, s3);
        const int px1 = wave_shr1(s1, NEG2_16), px2 = wave_shr1(s2, NEG2_16);
        const int f10 = px1 - o1_8 - l1, f20 = px2 - o2_8 - l2;
        const int f11 = max(px1, t10) - (o1_8 + e1_8) - l1, f21 = max(px2, t20) - (o2_8 + e2_8) - l2;
        const int htl0 = wave_shr1(htm1, NEG16);
        const int k30 = maxu16(maxu16(ht0 + 2, f10 + 1), f20), k31 = maxu16(maxu16(ht1 + 2, f11 + 1), f21);
        const int h0 = k30 & ~7, h1 = k31 & ~7;
        unsigned d0 = ((unsigned)(E1t0 | E2t0) & 3u) | (((unsigned)k20 & 3u) << 2) | (((unsigned)k30 & 3u) << 4);
        unsigned d1 = ((unsigned)(E1t1 | E2t1) & 3u) | (((unsigned)k21 & 3u) << 2) | (((unsigned)k31 & 3u) << 4);
        d0 |= (((unsigned)(htl0 - oe1_8 - f10)) >> 25) & 64u; d0 |= (((unsigned)(htl0 - oe2_8 - f20)) >> 24) & 128u;
        d1 |= (((unsigned)(htm0 - oe1_8 - f11)) >> 25) & 64u; d1 |= (((unsigned)(htm0 - oe2_8 - f21)) >> 24) & 128u;
        const int rb = __builtin_amdgcn_readlane(s3, 63);
        const unsigned long long mx0 = __ballot(htm0 == rb), mx1 = __ballot(htm1 == rb);
        left = beg + min(mx0 ? 2 * (int)__builtin_ctzll(mx0) : 256, mx1 ? 2 * (int)__builtin_ctzll(mx1) + 1 : 256);
        right = beg + max(mx0 ? 2 * (63 - (int)__builtin_clzll(mx0)) : -1, mx1 ? 2 * (63 - (int)__builtin_clzll(mx1)) + 1 : -1);
        int vH0 = maxu16(selm(am0, h0, vneg), FLOOR16), vE10 = selm(am0, E1c0, vneg), vE20 = selm(am0, E2c0, vneg);
        int vH1 = maxu16(selm(am1, h1, vneg), FLOOR16), vE11 = selm(am1, E1c1, vneg), vE21 = selm(am1, E2c1, vneg);
        if ((unsigned)(rb - RB_LO16) > (unsigned)rb_span) {
          const int m1 = rb - BIAS16, fl1 = FLOOR16 + max(m1, 0);
          nb8 += m1; if (rb < GLO16) punt = 1;
          vH0 = selm(am0, maxu16(h0, fl1) - m1, vneg); vE10 = selm(am0, maxu16(E1c0, fl1) - m1, vneg); vE20 = selm(am0, maxu16(E2c0, fl1) - m1, vneg);
          vH1 = selm(am1, maxu16(h1, fl1) - m1, vneg); vE11 = selm(am1, maxu16(E1c1, fl1) - m1, vneg); vE21 = selm(am1, maxu16(E2c1, fl1) - m1, vneg);
        }
        gacc = minu16(minu16(gacc, vH0 - (ZHI16 + 1)), vH1 - (ZHI16 + 1));
        *(unsigned short*)(D + (voff + (unsigned)lane)) = (unsigned short)((d0 & 0xffu) | ((d1 & 0xffu) << 8));
        rs ^= 1;
        { const int cb = PADL + c0l;
          LH[rs][cb] = (unsigned short)vH0; LE1[rs][cb] = (unsigned short)vE10; LE2[rs][cb] = (unsigned short)vE20;
          LH[rs][cb + 1] = (unsigned short)vH1; LE1[rs][cb + 1] = (unsigned short)vE11; LE2[rs][cb + 1] = (unsigned short)vE21; }
        pvk = -4096; in_ring = 1;
      }
      asm("v_writelane_b32 %0, %1, m0" : "+v"(recv) : "s"(beg | (wd << 16)), "{m0}"(li));   // (lane select in m0: one SGPR operand at most)
      voff += DSTRIDE; asm volatile("" : "+v"(voff));                // (a vector offset under a scalar base: no 64-bit pointer per row)
      u_left = left; u_right = right; u_b8 = nb8; ncell += wd;
    }
    if (lane < cnt) rowrec[ib + lane] = recv;                      // (a declined read's records are never read)
    li0 = 0;
  }
  // a value the 16-bit cells cannot hold exactly: k_poa hands such a read to its 32-bit pass
  if (Q0run < 0 || punt != 0 || __builtin_amdgcn_ballot_w64((unsigned)(gacc & 0xffff) < (unsigned)(GLO16 - ZHI16 - 1)) != 0) return -1;
  // ---- end cell: column Q1 of the last row
  {
    if (Q1 < u_beg || Q1 > u_end) return -1;
    int hq;
    if (pvk >= 0) hq = __builtin_amdgcn_readlane(pH, Q1 - u_beg);
    else hq = wave_first((int)LH[rs][PADL + Q1 - u_beg]);
    if (hq < ZLO16) return -1;
  }
  WSYNC();                                                         // direction bytes and row records are read by other lanes; the ring becomes windows
  // ---- traceback: k_poa's state machine, 64 rows per block; every row's one predecessor is the row above, its node row + 1
  int rc = 0;
  {
    uint8_t* const WD = &L.win[0];
    int i = Q0, j = Q1, st = 0;                                    // st: 0 H, 1 Ht, 2 E1, 3 E2, 4 F1, 5 F2
    while (!(i == 0 && j == 0) && rc == 0) {
      const int it = i, jt = j;
      const int rk = it - lane;
      const int ic = max(rk, 0);
      const int rec = rowrec[ic];
      const int b = rec & 0xffff, e = b + (rec >> 16) - 1, ro = ic * DSTRIDE;
      int a0 = ro + (jt - lane - 8 - b);
      a0 = min(max(a0, 0), (int)a.dbytes - 32) & ~3;
      const int w0 = a0 - ro + b;                                  // column of window byte 0
      {
        const uint32_t* src = (const uint32_t*)(D + a0);
        const uint4 x0 = make_uint4(src[0], src[1], src[2], src[3]), x1 = make_uint4(src[4], src[5], src[6], src[7]);
        uint4* wd_ = (uint4*)(WD + lane * 32); wd_[0] = x0; wd_[1] = x1;
      }
      WSYNC();
      for (;;) {
        const int s = it - i;                                      // lane s holds the current row
        const int jk = j - (lane - s);
        const bool inb = rk >= 0 && lane >= s && jk >= b && jk <= e;
        const int wo = jk - w0;
        const bool hit = inb && wo >= 0 && wo < 32;
        const unsigned d = WD[lane * 32 + min(max(wo, 0), 31)];
        if (st == 0 && i > 0 && j > 0) {
          const bool ok = hit && rk >= 1 && jk >= 1 && ((d >> 2) & 15u) == 10u;
          const unsigned long long bal = __ballot(ok) >> s;
          int m = (~bal) ? __builtin_ctzll(~bal) : 64;
          m = min(m, 64 - s);
          if (lane >= s && lane < s + m) vq[jk - 1] = (uint16_t)(rk + 1);
          i -= m; j -= m;
          if (i == 0 && j == 0) break;
          if (s + m >= 64) break;                                  // block used up: fetch the next 64 rows
        }
        const int cl = it - i;                                     // the current cell (i, j) sits in lane cl
        if (!wave_bcast((int)inb, cl)) { rc = -2; break; }
        unsigned db;
        if (wave_bcast((int)hit, cl)) db = (unsigned)wave_bcast((int)d, cl);
        else db = D[(size_t)i * DSTRIDE + (j - wave_bcast(b, cl))];   // the path drifted out of the window
        const unsigned c1 = (~db) & 1u, c2 = ((~db) >> 1) & 1u, hts = 2u - ((db >> 2) & 3u), hs = 2u - ((db >> 4) & 3u), f1x = (db >> 6) & 1u, f2x = db >> 7;
        for (bool same = true; same;) {
          if (st == 0) { st = hs == 0 ? 1 : (hs == 1 ? 4 : 5); }
          else if (st == 1) {
            if (hts == 0) { if (j < 1) { rc = -2; break; } if (lane == 0) vq[j - 1] = (uint16_t)(i + 1); --i; --j; st = 0; same = false; }
            else st = hts == 1 ? 2 : 3;
          }
          else if (st == 2) { --i; st = c1 ? 2 : 0; same = false; }
          else if (st == 3) { --i; st = c2 ? 3 : 0; same = false; }
          else { if (j < 1) { rc = -2; break; } if (lane == 0) vq[j - 1] = 0xffff; st = st == 4 ? (f1x ? 4 : 1) : (f2x ? 5 : 1); --j; same = false; }
        }
        if (rc < 0) break;
        if (i == 0 && j == 0) break;
        if (i < 0 || j < 0) { rc = -2; break; }
        const int drift = (jt - j) - (it - i);
        if (it - i >= 64 || drift > 4 || drift < -20) break;
      }
      WSYNC();
    }
  }
  return rc < 0 ? -1 : ncell;
}

// 6 waves per SIMD: what k_poa's slot count (24 waves per CU) lets be resident anyway; 73 VGPRs, nothing spilled, no scratch,
// 3 984 bytes of LDS.
// Bounded to 8 (64 VGPRs, 5 spilled) it measured the same
#ifndef C3_PAIR_WAVES
#define C3_PAIR_WAVES 6
#endif
__global__ __launch_bounds__(64, C3_PAIR_WAVES) void k_poa_pair(PoaPairArgs a) {
  const int lane = wave_lane();
  const int slot = blockIdx.x;
  uint8_t* const D = (uint8_t*)a.cellsb + (size_t)slot * (size_t)a.dstride;
  int* const rowrec = a.ibase + (size_t)slot * C3_POA_NI * (size_t)a.Ncap + C3_POA_I_ROWM * (size_t)a.Ncap;      // k_poa's rowm (3 * Ncap ints)
  for (;;) {
    int wi = 0;
    if (lane == 0) wi = atomicAdd(&a.cnt->pair_queue, 1);
    wi = wave_first(wi);
    if (wi >= a.n_work) break;
    const int rid = a.work[wi];
    const C3Info* info = &a.info[rid];
    const int ns = wave_first(info->n_sub);
    int cells = -1;
    if (ns >= 2) {
      const int qb0 = wave_first(info->sub_beg[0]), Q0 = wave_first(info->sub_end[0]) - qb0;
      const int qb1 = wave_first(info->sub_beg[1]), Q1 = wave_first(info->sub_end[1]) - qb1;
      cells = pair_align(a, a.b.pk + a.b.woff[rid], qb0, Q0, qb1, Q1, D, rowrec, a.vq + a.b.off[rid] + qb1, lane);
    }
    WSYNC();
    // (no divergent store right before the back edge of the persistent loop: the barrier follows it)
    if (lane == 0 && ns >= 2) {
      if (cells > 0) { a.cells[rid] = cells; a.done[rid] = 1; atomicAdd(&a.cnt->n_pair, 1); }
      else atomicAdd(&a.cnt->n_pair_declined, 1);
    }
    WSYNC();
  }
}

extern "C" void c3k_launch_poa_pair(const PoaPairArgs* a, int slots, hipStream_t stream) {
  hipLaunchKernelGGL(k_poa_pair, dim3(slots), dim3(64), 0, stream, *a);
}
