// inflate_device.h -- GZIP members (RFC 1952) around DEFLATE streams (RFC 1951) decoded on the device: the Parquet codec GZIP (2), which the `parquet` crate
// (arrow-rs 50, not part of the reference tree) hands to flate2's MultiGzDecoder on the CPU.  Restated from the published formats: one or more members per
// page (header with FEXTRA / FNAME / FCOMMENT / FHCRC, stored / fixed / dynamic Huffman blocks, CRC-32 and ISIZE trailer), no zlib wrapper, no raw streams.
//
// One workgroup of two waves per page, a producer / consumer pair.  A DEFLATE stream is sequential (a block's end is known only once its last symbol is
// decoded), so the pages of a read are the parallelism, as for Zstandard.  Wave 0 decodes: every value it steers by is wave-uniform (read from LDS and
// pinned to the scalar unit), each symbol with its extra bits is resolved by one read of a primary lookup table (10 bits for literals / lengths, 8 bits
// for distances; longer codes take a canonical walk), bits come from a 64-bit register window refilled from an LDS window of the input.  It appends
// sequences (literal count, match length, distance) and literal bytes to one half of a double-buffered LDS queue.  Wave 1 drains the other half with 64
// lanes into an LDS ring of the latest 32 KB of output (matches reaching further back read the flushed output in HBM, as lz4_decode does), flushes the ring
// with 16-byte stores and folds every flushed byte into the member's CRC-32 (slicing by 4 per lane, lanes combined by GF(2) shifts).  The two waves meet
// at one barrier pair per batch.
#pragma once
#include "device_utils.h"

namespace dfgpu {
namespace gz {

constexpr uint32_t GZ_RING = 32768, GZ_WIN_W = 1024, GZ_NSEQ = 192, GZ_NLIT = 768, GZ_LBITS = 10, GZ_DBITS = 8;
enum : uint32_t { SEQ_MATCH = 0, SEQ_STORED = 1, SEQ_MEND = 2 };
struct Seq { uint32_t a, len, b; };     // a = literal count | kind << 24; MATCH: len (0 = literals only), b = distance; STORED: len, b = input offset; MEND: b = CRC-32
struct Lds {
  uint8_t ring[GZ_RING];                // latest output
  uint32_t win[GZ_WIN_W];               // input words [w_hi - GZ_WIN_W, w_hi)
  Seq seq[2][GZ_NSEQ]; uint8_t lit[2][GZ_NLIT];
  uint32_t ltab[1 << GZ_LBITS], dtab[1 << GZ_DBITS], ctab[128];       // n | extra << 4 | kind << 8 | value << 16; n = 0: longer code (canonical walk) or none
  uint16_t lsym[288], dsym[32], csym[19], lcnt[16], dcnt[16], ccnt[16];
  uint8_t lens[320];
  uint32_t crc[4][256], x16[65];        // slicing-by-4 tables; x16[j] = x^(128 j) mod P (a shift by 16 j bytes)
  uint32_t n[2], done, bad;
};

// CRC-32 (reflected, P = 0xEDB88320) helpers, the arithmetic of zlib's crc32_combine: a(x) b(x) mod P, a != 0
__host__ __device__ constexpr uint32_t mulp(uint32_t a, uint32_t b) {
  if (!a) return 0;
  uint32_t m = 1u << 31, p = 0;
  for (;;) { if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; } m >>= 1; b = b & 1 ? (b >> 1) ^ 0xEDB88320u : b >> 1; }
  return p;
}
struct CrcTabs { uint32_t t[4][256]; uint32_t x16[65]; };
constexpr CrcTabs make_crc_tabs() {
  CrcTabs r{};
  for (uint32_t n = 0; n < 256; n++) { uint32_t c = n; for (int k = 0; k < 8; k++) c = c & 1 ? (c >> 1) ^ 0xEDB88320u : c >> 1; r.t[0][n] = c; }
  for (int k = 1; k < 4; k++) for (uint32_t n = 0; n < 256; n++) r.t[k][n] = (r.t[k - 1][n] >> 8) ^ r.t[0][r.t[k - 1][n] & 0xff];
  uint32_t x = 1u << 30;                                        // x^1
  for (int k = 0; k < 7; k++) x = mulp(x, x);                   // x^128
  r.x16[0] = 1u << 31; for (int j = 1; j <= 64; j++) r.x16[j] = mulp(r.x16[j - 1], x);
  return r;
}
__device__ const CrcTabs GZ_CRC = make_crc_tabs();

__device__ const uint16_t GZ_LBASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__device__ const uint8_t GZ_LEXT[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__device__ const uint16_t GZ_DBASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__device__ const uint8_t GZ_CLORD[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
__device__ const uint8_t GZ_DEXT[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

#define gz_u(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))

// table entry of symbol s with a code of n bits; kind 0 literal / length, 1 distance, 2 code length.  Entry kinds: 0 literal, 1 length or distance, 2 end of block, 3 invalid
__device__ inline uint32_t entry(int kind, uint32_t s, uint32_t n) {
  if (kind == 2) return n | (s << 16);
  if (kind == 1) return s < 30 ? n | ((uint32_t)GZ_DEXT[s] << 4) | (1u << 8) | ((uint32_t)GZ_DBASE[s] << 16) : n | (3u << 8);
  if (s < 256) return n | (s << 16);
  if (s == 256) return n | (2u << 8);
  return s <= 285 ? n | ((uint32_t)GZ_LEXT[s - 257] << 4) | (1u << 8) | ((uint32_t)GZ_LBASE[s - 257] << 16) : n | (3u << 8);
}

// Canonical code of lens[0, n) -> primary table tab (1 << tb entries) and, for codes longer than tb, the count / symbol lists of the canonical walk.  All 64
// lanes of the decoder wave: lane L (1..15) owns the codes of length L.  false for an over-subscribed set, or an incomplete one with more than one code (a lone
// code and an empty set are accepted, as miniz_oxide and zlib accept them; using a code they lack is an error when it happens).
__device__ inline bool build(const uint8_t* lens, int n, uint32_t* tab, int tb, uint16_t* cnt, uint16_t* sym, int kind, uint32_t lane) {
  uint32_t c = 0;
  for (int s = 0; s < n; s++) c += lens[s] == lane ? 1u : 0u;
  if (lane == 0 || lane > 15) c = 0;
  int left = 1; uint32_t used = 0, offs = 0, code = 0, prev = 0, my_offs = 0, my_code = 0;
  for (uint32_t L = 1; L <= 15; L++) {
    code = (code + prev) << 1;
    if (lane == L) { my_offs = offs; my_code = code; }
    prev = gz_u(__builtin_amdgcn_readlane((int)c, (int)L));
    left = (left << 1) - (int)prev; if (left < 0) return false;
    used += prev; offs += prev;
  }
  if (left > 0 && used > 1) return false;
  if (lane < 16) cnt[lane] = (uint16_t)c;
  for (uint32_t i = lane; i < (1u << tb); i += 64) tab[i] = 0;
  __builtin_amdgcn_wave_barrier();
  if (lane >= 1 && lane <= 15 && c) {
    uint32_t k = 0;
    for (int s = 0; s < n; s++) if (lens[s] == lane) {
      sym[my_offs + k] = (uint16_t)s;
      if ((int)lane <= tb) { const uint32_t r = __brev(my_code + k) >> (32 - lane), e = entry(kind, (uint32_t)s, lane); for (uint32_t i = r; i < (1u << tb); i += 1u << lane) tab[i] = e; }
      k++;
    }
  }
  __builtin_amdgcn_wave_barrier();
  return true;
}
// a code longer than the primary table: the canonical walk (RFC 1951 3.2.2) over the next 15 bits of w; 0 when no code matches
__device__ inline uint32_t walk(uint64_t w, const uint16_t* cnt, const uint16_t* sym, int kind) {
  int code = 0, first = 0, index = 0;
  for (uint32_t len = 1; len <= 15; len++) {
    code |= (int)((w >> (len - 1)) & 1);
    const int count = (int)gz_u(cnt[len]);
    if (code - first < count && code >= first) return entry(kind, gz_u(sym[index + code - first]), len);
    index += count; first += count; first <<= 1; code <<= 1;
  }
  return 0;
}

// Decode the GZIP members src[0, csize) into dst[0, usize).  Called by both waves of a 128-thread workgroup; false when the page is malformed (any bit of it:
// header, block, code set, symbol, distance, stored length, truncation, trailing bytes, CRC-32, ISIZE, FHCRC, total size).
__device__ inline bool inflate_page(Lds* L, const uint8_t* src, uint32_t csize, uint8_t* dst, uint32_t usize) {
  constexpr uint32_t RM = GZ_RING - 1, WM = GZ_WIN_W - 1;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = gz_u(tid >> 6);
  for (uint32_t i = tid; i < 4 * 256; i += 128) L->crc[i >> 8][i & 255] = GZ_CRC.t[i >> 8][i & 255];
  for (uint32_t i = tid; i < 65; i += 128) L->x16[i] = GZ_CRC.x16[i];
  if (tid == 0) { L->n[0] = L->n[1] = 0; L->done = 0; L->bad = 0; }
  __syncthreads();

  // ---- decoder state (wave 0; every value wave-uniform)
  const uint32_t lead = (uint32_t)((uintptr_t)src & 15); const uint4* q4 = (const uint4*)(src - lead);
  const uint64_t end_bits = ((uint64_t)lead + csize) * 8;
  uint64_t bb = 0; uint32_t nb = 0, wi = 0, w_hi = 0;
  uint32_t st = 0, bfinal = 0, out = 0, mstart = 0; int tabs = -1;    // st: 0 member header, 1 block header, 2 Huffman block, 3 trailer, 4 done; tabs: 1 fixed tables loaded
  auto load_more = [&]() {                      // input words [w_hi, w_hi + 512) into the window; words past the input read as zero
    for (uint32_t g = lane; g < 128; g += 64) { const uint32_t w = w_hi + 4 * g; uint4 v = make_uint4(0, 0, 0, 0); if ((uint64_t)w * 4 < (uint64_t)lead + csize) v = q4[w >> 2]; *(uint4*)&L->win[w & WM] = v; }
    w_hi += 512; __builtin_amdgcn_wave_barrier();
  };
  auto refill = [&]() { if (nb <= 32) { if (wi + 1 >= w_hi) load_more(); bb |= (uint64_t)gz_u(L->win[wi & WM]) << nb; wi++; nb += 32; } };
  auto pos = [&]() -> uint64_t { return (uint64_t)wi * 32 - nb; };        // bits consumed, from the aligned base
  auto bits = [&](uint32_t n) -> uint32_t { refill(); const uint32_t v = (uint32_t)(bb & ((1ull << n) - 1)); bb >>= n; nb -= n; return v; };
  auto seek = [&](uint64_t bit) { wi = (uint32_t)(bit >> 5); w_hi = wi & ~3u; load_more(); const uint32_t sh = (uint32_t)(bit & 31); bb = (uint64_t)gz_u(L->win[wi & WM]) >> sh; nb = 32 - sh; wi++; };
  auto align = [&]() { const uint32_t k = nb & 7; bb >>= k; nb -= k; };
  uint32_t hcrc = 0;
  auto hbyte = [&](bool& ok) -> uint32_t { if (pos() + 8 > end_bits) { ok = false; return 0; } const uint32_t b = bits(8); hcrc = gz_u(L->crc[0][(hcrc ^ b) & 0xff]) ^ (hcrc >> 8); return b; };
  // ---- drain state (wave 1)
  uint32_t dout = 0, flushed = 0, fenced = 0, cpos = 0, crun = 0; bool dbad = false;
  const bool dst16 = ((uintptr_t)dst & 15) == 0;
  auto crc_upd = [&](uint32_t upto, bool fin) {   // fold output [cpos, upto) into crun; without `fin` up to 15 bytes wait for the next call
    while ((cpos & 15) && cpos < upto) { const uint32_t b = L->ring[cpos & RM]; const uint32_t c = ~crun; crun = ~(L->crc[0][(c ^ b) & 0xff] ^ (c >> 8)); cpos++; }
    while (upto - cpos >= 16) {
      const uint32_t np = (upto - cpos) >> 4, n = np < 64 ? np : 64; uint32_t part = 0;
      if (lane < n) {
        const uint4 v = *(const uint4*)(L->ring + ((cpos + 16 * lane) & RM)); uint32_t c = 0xFFFFFFFFu;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) { c ^= w[k]; c = L->crc[3][c & 0xff] ^ L->crc[2][(c >> 8) & 0xff] ^ L->crc[1][(c >> 16) & 0xff] ^ L->crc[0][c >> 24]; }
        part = mulp(L->x16[n - 1 - lane], ~c);
      }
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) part ^= (uint32_t)__shfl_xor((int)part, s, 64);
      crun = mulp(L->x16[n], gz_u(crun)) ^ gz_u(part); cpos += 16 * n;
    }
    if (fin) while (cpos < upto) { const uint32_t b = L->ring[cpos & RM]; const uint32_t c = ~crun; crun = ~(L->crc[0][(c ^ b) & 0xff] ^ (c >> 8)); cpos++; }
  };
  auto flush = [&](uint32_t upto, bool all) {     // ring[flushed, upto) -> dst (the lz4_decode flush); the CRC first, while the bytes are still in the ring
    __builtin_amdgcn_wave_barrier();
    crc_upd(upto, false);
    uint32_t a = flushed;
    if (!dst16) { if (all || upto - a >= 4096) { for (uint32_t q = a + lane; q < upto; q += 64) dst[q] = L->ring[q & RM]; flushed = upto; } return; }
    const uint32_t a16 = (a + 15u) & ~15u, e16 = upto & ~15u;
    if (a16 > a) { const uint32_t h = a16 < upto ? a16 : upto; for (uint32_t q = a + lane; q < h; q += 64) dst[q] = L->ring[q & RM]; a = h; }
    if (e16 > a) { for (uint32_t q = a + lane * 16; q < e16; q += 1024) *(uint4*)(dst + q) = *(const uint4*)(L->ring + (q & RM)); a = e16; }
    if (all && upto > a) { for (uint32_t q = a + lane; q < upto; q += 64) dst[q] = L->ring[q & RM]; a = upto; }
    flushed = a;
  };
  auto room = [&](uint32_t c) { if (dout + c - flushed > GZ_RING - 64) flush(dout, false); };

  if (wave == 0) seek((uint64_t)lead * 8);        // the stream starts `lead` bytes into the first aligned input word
  uint32_t cur = 0;
  for (;;) {
    if (wave == 0) {
      if (!gz_u(L->done)) {
        // ---- decode one batch into half `cur`
        Seq* sq = L->seq[cur]; uint8_t* lt = L->lit[cur];
        uint32_t ns = 0, nl = 0, pend = 0; bool bad = false;
        auto emit = [&](uint32_t kind, uint32_t len, uint32_t b) { if (lane == 0) sq[ns] = Seq{pend | (kind << 24), len, b}; ns++; pend = 0; };
        while (!bad && st != 4 && ns + 3 <= GZ_NSEQ && nl + 1 <= GZ_NLIT) {
          if (st == 0) {                                 // member header
            bool ok = true; hcrc = 0xFFFFFFFFu;
            const uint32_t id1 = hbyte(ok), id2 = hbyte(ok), cm = hbyte(ok), flg = hbyte(ok);
            for (int k = 0; k < 6; k++) hbyte(ok);       // MTIME, XFL, OS
            if (!ok || id1 != 0x1f || id2 != 0x8b || cm != 8 || (flg & 0xe0)) { bad = true; break; }
            if (flg & 4) { const uint32_t x0 = hbyte(ok), x1 = hbyte(ok); uint32_t xl = x0 | (x1 << 8); while (ok && xl--) hbyte(ok); }
            if (flg & 8) { while (ok && hbyte(ok) != 0) {} }
            if (flg & 16) { while (ok && hbyte(ok) != 0) {} }
            if (flg & 2) { const uint32_t want = ~hcrc & 0xffff; const uint32_t h0 = hbyte(ok), h1 = hbyte(ok); if (ok && (h0 | (h1 << 8)) != want) ok = false; }
            if (!ok) { bad = true; break; }
            mstart = out; st = 1; continue;
          }
          if (st == 1) {                                 // block header
            if (pos() + 3 > end_bits) { bad = true; break; }
            const uint32_t h = bits(3); bfinal = h & 1; const uint32_t bt = h >> 1;
            if (bt == 0) {                               // stored: LEN / NLEN, then LEN bytes copied from the input by the drain
              align(); const uint32_t ln = bits(16), nln = bits(16);
              const uint64_t bp = pos() / 8 - lead;
              if (pos() > end_bits || ln != (~nln & 0xffff) || bp + ln > csize || out + ln > usize) { bad = true; break; }
              if (ln) { emit(SEQ_STORED, ln, (uint32_t)bp); out += ln; }
              seek(pos() + (uint64_t)ln * 8);
              st = bfinal ? 3 : 1; continue;
            }
            if (bt == 1) {                               // fixed Huffman codes
              if (tabs != 1) {
                for (uint32_t s = lane; s < 320; s += 64) L->lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
                __builtin_amdgcn_wave_barrier();
                build(L->lens, 288, L->ltab, GZ_LBITS, L->lcnt, L->lsym, 0, lane); build(L->lens + 288, 32, L->dtab, GZ_DBITS, L->dcnt, L->dsym, 1, lane);
                tabs = 1;
              }
              st = 2; continue;
            }
            if (bt != 2) { bad = true; break; }          // BTYPE 3
            const uint32_t hlit = bits(5) + 257, hdist = bits(5) + 1, hclen = bits(4) + 4;
            if (hlit > 286 || hdist > 30) { bad = true; break; }
            if (lane < 19) L->lens[300 + lane] = 0;
            __builtin_amdgcn_wave_barrier();
            for (uint32_t k = 0; k < hclen; k++) { const uint32_t v = bits(3); if (lane == 0) L->lens[300 + GZ_CLORD[k]] = (uint8_t)v; }
            __builtin_amdgcn_wave_barrier();
            if (!build(L->lens + 300, 19, L->ctab, 7, L->ccnt, L->csym, 2, lane)) { bad = true; break; }
            tabs = 0;
            uint32_t k = 0, last = 0xFFu;
            while (k < hlit + hdist) {
              refill(); const uint32_t e = gz_u(L->ctab[bb & 127]); const uint32_t n = e & 15;
              if (!n) { bad = true; break; }
              bb >>= n; nb -= n; const uint32_t sym = e >> 16;
              if (sym < 16) { if (lane == 0) L->lens[k] = (uint8_t)sym; last = sym; k++; continue; }
              uint32_t rep, val;
              if (sym == 16) { if (last == 0xFFu) { bad = true; break; } rep = 3 + bits(2); val = last; }
              else if (sym == 17) { rep = 3 + bits(3); val = 0; } else { rep = 11 + bits(7); val = 0; }
              if (k + rep > hlit + hdist) { bad = true; break; }
              for (uint32_t i = lane; i < rep; i += 64) L->lens[k + i] = (uint8_t)val;
              k += rep; last = val;
            }
            if (bad) break;
            __builtin_amdgcn_wave_barrier();
            if (gz_u(L->lens[256]) == 0) { bad = true; break; }
            // the distance lengths move behind the 288 literal / length slots
            uint8_t dl = 0; if (lane < hdist) dl = L->lens[hlit + lane];
            __builtin_amdgcn_wave_barrier();
            for (uint32_t s = hlit + lane; s < 320; s += 64) L->lens[s] = 0;
            __builtin_amdgcn_wave_barrier();
            if (lane < 32) L->lens[288 + lane] = lane < hdist ? dl : 0;
            __builtin_amdgcn_wave_barrier();
            if (pos() > end_bits || !build(L->lens, (int)hlit, L->ltab, GZ_LBITS, L->lcnt, L->lsym, 0, lane) || !build(L->lens + 288, (int)hdist, L->dtab, GZ_DBITS, L->dcnt, L->dsym, 1, lane)) { bad = true; break; }
            st = 2; continue;
          }
          if (st == 2) {                                 // Huffman block: symbols until the batch is full or the block ends
            while (ns + 3 <= GZ_NSEQ && nl < GZ_NLIT) {
              refill();
              uint32_t e = gz_u(L->ltab[bb & ((1u << GZ_LBITS) - 1)]);
              if (!(e & 15)) { e = walk(bb, L->lcnt, L->lsym, 0); if (!e) { bad = true; break; } }
              const uint32_t n = e & 15, kind = (e >> 8) & 3;
              if (kind == 0) {
                if (out >= usize) { bad = true; break; }
                if (lane == 0) lt[nl] = (uint8_t)(e >> 16);
                nl++; pend++; out++; bb >>= n; nb -= n; continue;
              }
              if (kind == 2) { bb >>= n; nb -= n; st = bfinal ? 3 : 1; break; }
              if (kind == 3) { bad = true; break; }
              const uint32_t ex = (e >> 4) & 15, len = (e >> 16) + (uint32_t)((bb >> n) & ((1u << ex) - 1)); bb >>= n + ex; nb -= n + ex;
              refill();
              uint32_t d = gz_u(L->dtab[bb & ((1u << GZ_DBITS) - 1)]);
              if (!(d & 15)) { d = walk(bb, L->dcnt, L->dsym, 1); if (!d) { bad = true; break; } }
              if (((d >> 8) & 3) != 1) { bad = true; break; }
              const uint32_t dn = d & 15, dx = (d >> 4) & 15, dist = (d >> 16) + (uint32_t)((bb >> dn) & ((1u << dx) - 1)); bb >>= dn + dx; nb -= dn + dx;
              if (dist > out - mstart || len > usize - out) { bad = true; break; }
              emit(SEQ_MATCH, len, dist); out += len;
            }
            if (!bad && pos() > end_bits) bad = true;
            continue;
          }
          if (st == 3) {                                 // trailer: CRC-32, ISIZE; then another member or the end of the page
            align(); const uint32_t c0 = bits(16), c1 = bits(16), s0 = bits(16), s1 = bits(16); const uint32_t crc = c0 | (c1 << 16), isz = s0 | (s1 << 16);
            if (pos() > end_bits || isz != out - mstart) { bad = true; break; }
            emit(SEQ_MEND, 0, crc);
            st = pos() == end_bits ? 4 : 0; continue;
          }
        }
        if (pend) emit(SEQ_MATCH, 0, 0);
        if (!bad && st == 4 && out != usize) bad = true;
        if (lane == 0) { L->n[cur] = bad ? 0u : ns; if (bad) L->bad = 1; if (bad || st == 4) L->done = 1; }
      } else if (lane == 0) L->n[cur] = 0;
    } else {
      // ---- drain the half filled in the previous round
      const uint32_t h = cur ^ 1u, ns = gz_u(L->n[h]); const Seq* sq = L->seq[h]; const uint8_t* lt = L->lit[h]; uint32_t lp = 0;
      for (uint32_t i = 0; i < ns; i++) {
        const uint32_t a = gz_u(sq[i].a), len = gz_u(sq[i].len), b = gz_u(sq[i].b), kind = a >> 24, ll = a & 0xFFFFFFu;
        if (ll) { room(ll); for (uint32_t k = lane; k < ll; k += 64) L->ring[(dout + k) & RM] = lt[lp + k]; dout += ll; lp += ll; }
        if (kind == SEQ_MEND) { crc_upd(dout, true); if (crun != b) dbad = true; crun = 0; continue; }
        if (kind == SEQ_STORED) {
          uint32_t n = len, at = b;
          while (n) { const uint32_t c = n < 8192 ? n : 8192; room(c); for (uint32_t k = lane; k < c; k += 64) L->ring[(dout + k) & RM] = src[at + k]; dout += c; at += c; n -= c; }
          continue;
        }
        if (!len) continue;
        room(len); __builtin_amdgcn_wave_barrier();
        if (b + len <= GZ_RING) {                       // the source lies in the ring
          const uint32_t from = dout - b;
          if (b >= len) { for (uint32_t k = lane; k < len; k += 64) L->ring[(dout + k) & RM] = L->ring[(from + k) & RM]; }
          else if (b == 1) { const uint8_t v = L->ring[from & RM]; for (uint32_t k = lane; k < len; k += 64) L->ring[(dout + k) & RM] = v; }
          else for (uint32_t k = lane; k < len; k += 64) { const uint8_t v = L->ring[(from + k % b) & RM]; __builtin_amdgcn_wave_barrier(); L->ring[(dout + k) & RM] = v; }
        } else {                                         // further back than the ring: everything written so far leaves for HBM, one wait, then the source is read there
          if (dout - b + (len < b ? len : b) > fenced) { flush(dout, true); __threadfence_block(); fenced = dout; }
          for (uint32_t k = lane; k < len; k += 64) L->ring[(dout + k) & RM] = dst[dout - b + (b >= len ? k : k % b)];
        }
        dout += len; __builtin_amdgcn_wave_barrier();
      }
    }
    __syncthreads();
    const bool stop = L->done && L->n[cur] == 0;
    __syncthreads();
    if (stop) break;
    cur ^= 1u;
  }
  if (wave == 1) flush(dout, true);
  const bool bad = L->bad != 0;
  return !(bad || (wave == 1 && dbad));
}

}  // namespace gz
}  // namespace dfgpu
