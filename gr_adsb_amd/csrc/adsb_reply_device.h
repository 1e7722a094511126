// adsb_reply_device.h -- the device code that more than one translation unit needs, each piece stated once: a record's flag
// constants, the CRC remainder table and the DF sets, the per-format sample read (|IQ|^2 of one sample as it lies in memory),
// and the syndrome and the parity pre-filter of a finished record's words.  Moved here, text unchanged, from adsb_device.h,
// which includes this header; adsb_softfec_device.h (ADSB_FLAG_FEC_SOFT) includes it too.  Device code only; it includes
// nothing and needs the includer's HIP device environment (the SIMT emulator of tests/sim provides its own).
#pragma once

namespace adsb {

enum RecFlags : unsigned {
  kDemod = 1u,     // eob inside the demod input: bits valid (demod.py:82)
  kKept = 2u,      // passed the re-trigger gate (framer.py:121)
  kNoMatch = 4u,   // placeholder whose long pulse did not match the preamble
  kPending = 8u,   // placeholder waiting for k_longrun
  kHead = 16u,     // shard mode: one of the first centres of the shard, delivered whether gated or not
  kLongHint = 32u, // CANDIDATE words only (long-aware gate, opt-in): the burst's first data bit is set = 112-bit reply
  // Mode S parity pre-filter (decoder.py:550-556 DF, :560-688 check_parity), kDemod only:
  kParityOk = 32u,   // DF 11/17/18/19 (parity/interrogator field) and the 24-bit syndrome is zero
  kLongFmt = 64u,    // DF 16/17/18/19/20/21/24: 112-bit reply (else the decoder reads 56 bits)
  kKnownDf = 128u,   // DF is one the reference decoder checks parity for (0,4,5,11,16-21,24)
  kDfShift = 8u,     // bits 8..12: the downlink format (first five bits, MSB first)
  kRecLongHint = 0x2000u,   // records of a long-aware context: this burst holds the gate for 119*sps, not 63*sps
  // opt-in Conservative error correction (k_fec; decoder.py:738-780), kDemod only:
  kFecFixed = 0x4000u,      // a 1-bit / 2-adjacent-bit error was repaired: bits and parity bits are those of the repaired reply
  kFecDf = 0x8000u,         // the decoder's repair would change the downlink format: bits left raw
  // opt-in aircraft table (k_air_*; decoder.py:576-665), kDemod records of the address/parity formats only.  They reuse the
  // values of kNoMatch / kPending, which never reach a delivered record (k_count drops such words):
  kApFec = 4u,      // AA unknown, but the decoder's Conservative repair accepts the reply (bits stay raw)
  kApKnown = 8u,    // AA announced by an earlier published reply
};

// x^j mod G, j = 0..111, G = x^24 + 0xFFF409 (decoder.py:268-269: the 25 coefficients spell 0x1FFF409).  The
// Mode S syndrome is linear in the message bits: bit i of an L-bit reply contributes x^(L-1-i) mod G, so
// compute_crc(bits[0:L-24]) ^ bits[L-24:L] (decoder.py:693-714 and its callers) is one XOR-reduction.
struct CrcTab { unsigned r[112]; };
constexpr CrcTab make_crc_tab() {
  CrcTab t{};
  unsigned v = 1;
  for (int j = 0; j < 112; ++j) {
    t.r[j] = v;
    v <<= 1;
    if (v & 0x1000000u) v ^= 0x1FFF409u;
  }
  return t;
}
// DF membership sets of decoder.py:565,604,636,669 as bit masks over the 5-bit DF
constexpr unsigned kDfShortSet = (1u << 0) | (1u << 4) | (1u << 5) | (1u << 11);
constexpr unsigned kDfLongSet = (1u << 16) | (1u << 17) | (1u << 18) | (1u << 19) | (1u << 20) | (1u << 21) | (1u << 24);
constexpr unsigned kDfPiSet = (1u << 11) | (1u << 17) | (1u << 18) | (1u << 19);

__device__ __forceinline__ float mag2f(float re, float im) {
  // two rounded products, one rounded add: never contracted into an FMA
  return __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
}

// int16 IQ: component -> float32 exactly, times `scale` (one rounded multiply), then |.|^2 as above
__device__ __forceinline__ float mag2_iq16(unsigned iq, float scale) {
  const float re = __fmul_rn((float)(short)(iq & 0xFFFFu), scale);
  const float im = __fmul_rn((float)(short)(iq >> 16), scale);
  return mag2f(re, im);
}

// 8-bit IQ (I in the low byte): MODE 3 = two's complement (cs8: HackRF, SDRplay): component = f32(int8) * scale;
// MODE 4 = offset binary (cu8: RTL-SDR): component = f32(2*u8 - 255) * scale, i.e. (u8 - 127.5) * 2*scale with
// the subtraction done exactly in integers.  One rounded multiply per component, then |.|^2 as above.
// MODE 5 = MODE 3 whose scale is a power of two (the usual int8 convention: x / 128): every intermediate of the
// float chain is then exact -- f32(i) * 2^-k, its square, the sum of two squares (< 2^15 * 2^-2k) -- so |IQ|^2 equals
// f32(i*i + q*q) * scale^2 bit for bit, and the tile loop takes the integer sum of squares from ONE v_dot4_i32_i8 per
// sample (body_convert); everything outside the tile loop converts as MODE 3 does.
constexpr int kModeSc8Pow2 = 5;
// MODE 6 = MODE 4 whose scale is a power of two (the RTL-SDR convention (u8 - 127.5) / 128 = (2*u8 - 255) * 2^-8): again every
// intermediate of the float chain is exact -- odd integers |c| <= 255 times 2^-k, their squares, the sum of two (< 2^18 *
// 2^-2k) -- and with x = u8 - 128 (the byte with its top bit flipped, read as a signed byte) c = 2x + 1, so
// c_i^2 + c_q^2 = 4 (x_i^2 + x_q^2 + x_i + x_q) + 2: two v_dot4c_i32_i8 per sample (x.x and x.1) in the tile loop (body_convert).
constexpr int kModeCu8Pow2 = 6;
template <int MODE>
__device__ __forceinline__ float mag2_iq8(unsigned iq, float scale) {
  if constexpr (MODE == 3 || MODE == kModeSc8Pow2) {
    const int i8 = (int)(signed char)(iq & 0xFFu), q8 = (int)(signed char)((iq >> 8) & 0xFFu);
    return mag2f(__fmul_rn((float)i8, scale), __fmul_rn((float)q8, scale));
  } else {
    // f32(2*u8 - 255) as 2*f32(u8) - 255: every step is exact (integers below 2^24), and it is one byte-to-float
    // conversion (v_cvt_f32_ubyteN, no extraction) and half a packed multiply-add per component instead of three
    // integer instructions and a conversion
    const float fi = (float)(iq & 0xFFu), fq = (float)((iq >> 8) & 0xFFu);
    const float ci = __builtin_fmaf(fi, 2.0f, -255.0f), cq = __builtin_fmaf(fq, 2.0f, -255.0f);
    return mag2f(__fmul_rn(ci, scale), __fmul_rn(cq, scale));
  }
}

constexpr bool mode_is_iq8(int mode) { return mode == 3 || mode == 4 || mode == 5 || mode == 6; }

// One sample as it lies in memory (RawSel<MODE>::type) and its conversion to |IQ|^2, kept apart so that a
// gather can be issued long before its value is needed.
template <int MODE> struct RawSel { using type = float; };
template <> struct RawSel<0> { using type = float2; };
template <> struct RawSel<2> { using type = unsigned; };
template <> struct RawSel<3> { using type = unsigned short; };
template <> struct RawSel<4> { using type = unsigned short; };
template <> struct RawSel<5> { using type = unsigned short; };
template <> struct RawSel<6> { using type = unsigned short; };

template <int MODE>
__device__ __forceinline__ typename RawSel<MODE>::type load_raw(const void* data, long long i) {
  return reinterpret_cast<const typename RawSel<MODE>::type*>(data)[i];
}
template <int MODE>
__device__ __forceinline__ float raw_mag2(typename RawSel<MODE>::type r, float scale) {
  if constexpr (MODE == 0) return mag2f(r.x, r.y);
  else if constexpr (MODE == 2) return mag2_iq16(r, scale);
  else if constexpr (mode_is_iq8(MODE)) return mag2_iq8<MODE>(r, scale);
  else return r;
}

template <int MODE>
__device__ __forceinline__ float load_sample(const void* data, long long i, float scale) {
  return raw_mag2<MODE>(load_raw<MODE>(data, i), scale);
}

template <int MODE>
__device__ __forceinline__ float xg(const void* data, long long n, long long i, float scale) {
  if (i < 0 || i >= n) return 0.0f;
  return load_sample<MODE>(data, i, scale);
}

// Mode S parity pre-filter of one finished record (one THREAD per record, in the tail: k_compact), from its packed
// bits: the same verdict as parity_prefilter above.  Syndrome = message polynomial mod G (decoder.py:693-714: CRC of
// the first L-24 bits XOR the last 24), byte-wise with the 256-entry table of v(x) * x^24 mod G.
struct Crc8Tab { unsigned t[256]; };
constexpr Crc8Tab make_crc8_tab() {
  Crc8Tab tab{};
  for (unsigned v = 0; v < 256; ++v) {
    unsigned c = v << 16;
    for (int k = 0; k < 8; ++k) {
      c <<= 1;
      if (c & 0x1000000u) c ^= 0x1FFF409u;
    }
    tab.t[v] = c & 0xFFFFFFu;
  }
  return tab;
}
__device__ __forceinline__ unsigned parity_flags_of(unsigned long long w2, unsigned long long w3) {
  static constexpr Crc8Tab tab = make_crc8_tab();
  const unsigned df = (unsigned)(w2 & 0xFFu) >> 3;                                         // decoder.py:551
  const unsigned dfb = 1u << df;
  const bool lng = (dfb & kDfLongSet) != 0, known = lng || (dfb & kDfShortSet) != 0;
  unsigned flags = df << kDfShift;
  if (lng) flags |= kLongFmt;
  if (known) flags |= kKnownDf;
  if (dfb & kDfPiSet) {                                                                     // decoder.py:625,679
    const int nb = lng ? 14 : 7;
    unsigned crc = 0u, last = 0u;
    for (int k = 0; k < nb; ++k) {
      const unsigned byte = (unsigned)((k < 8 ? (w2 >> (8 * k)) : (w3 >> (8 * (k - 8)))) & 0xFFu);
      if (k < nb - 3) crc = ((crc << 8) ^ tab.t[((crc >> 16) ^ byte) & 0xFFu]) & 0xFFFFFFu;
      else last = (last << 8) | byte;
    }
    if ((crc ^ last) == 0u) flags |= kParityOk;
  }
  return flags;
}
// the same syndrome, crc(bits[0:L-24]) ^ bits[L-24:L] for the first nb = L/8 bytes, for k_fec.  (parity_flags_of keeps its own
// loop: built on this function, k_compact and the one-workgroup tails compiled to different code -- same resources, not measured)
__device__ __forceinline__ unsigned syndrome_of(unsigned long long w2, unsigned long long w3, int nb) {
  static constexpr Crc8Tab tab = make_crc8_tab();
  unsigned crc = 0u, last = 0u;
  for (int k = 0; k < nb; ++k) {
    const unsigned byte = (unsigned)((k < 8 ? (w2 >> (8 * k)) : (w3 >> (8 * (k - 8)))) & 0xFFu);
    if (k < nb - 3) crc = ((crc << 8) ^ tab.t[((crc >> 16) ^ byte) & 0xFFu]) & 0xFFFFFFu;
    else last = (last << 8) | byte;
  }
  return crc ^ last;
}

}  // namespace adsb
