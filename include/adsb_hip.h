/* adsb_hip.h -- C ABI of libadsb_hip.so: the MI355X (gfx950) replacement for the framer + demod hot
 * path of mhostetter/gr-adsb.  Plain pointers and sizes only; no exceptions cross this boundary.
 *
 * The reference has no native code and therefore no FFI of its own: its two blocks are Python
 * gr.sync_block subclasses.  Each entry point below names the reference interface it replaces
 * (paths relative to the reference repo root):
 *
 *   adsb_create / adsb_destroy      framer.__init__ python/adsb/framer.py:37-65, demod.__init__ python/adsb/demod.py:35-54
 *   adsb_set_threshold              framer.set_threshold           python/adsb/framer.py:68-69
 *   adsb_framer_work[_passthrough]  framer.work()                  python/adsb/framer.py:72-182 (_passthrough: incl. :181 out0[:] = in0)
 *   adsb_demod_work                 demod.work()                   python/adsb/demod.py:57-136
 *   adsb_process_iq[_device]        complex_to_mag_squared -> framer -> demod as wired in
 *                                   examples/adsb_rx.py:180-196 (one canonical work() call per block)
 *   adsb_process_mag2[_device]      the same chain from the framer's float input onwards
 *   adsb_submit_*_device / adsb_wait   the same, up to ADSB_MAX_IN_FLIGHT calls in flight (no reference counterpart: pipelining)
 *   adsb_submit_format_host         the same fed from host memory: the SDR source -> framer chain of examples/adsb_rx.py:113-126,180-196
 *   adsb_last_confidence            demod.bit_confidence           python/adsb/demod.py:97-101
 *   adsb_set_soft_fec / adsb_last_soft / adsb_batch_last_soft   (no reference counterpart: decoder.py:772-776 "Brute Force" is unbuilt; SOFT REPAIR below)
 *   adsb_device_alloc / _free / _upload   (no reference counterpart: device memory for C / ctypes clients of the *_device entries)
 *   adsb_shard_device / adsb_shard_fixup / adsb_stitch   (no reference counterpart: overlapped time shards, host stitch)
 *   adsb_process_sharded_multi      the single process of examples/adsb_rx.py:242-268 (one flowgraph, one IQ source) fed to
 *                                   N devices: one host ring in, one stitched burst list out (ABI 5)
 *
 * Conventions: the caller owns every buffer it passes; the library owns device memory, pinned staging
 * and one HIP stream per context.  A context is single-threaded; different contexts may be used
 * concurrently.  Return value 0 = success, negative errno otherwise; when an output array is too
 * small the call returns -ENOSPC and *n_out holds the required count.  A threshold change takes
 * effect at the next call.  There is no CPU fallback: without a usable HIP device adsb_create fails.
 */
#ifndef ADSB_HIP_H
#define ADSB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ADSB_ABI_VERSION 5
#define ADSB_MAX_SPS 100 /* highest sample rate accepted: 100 Msps (tested up to and including it against the reference) */
#ifndef ADSB_MAX_IN_FLIGHT
#define ADSB_MAX_IN_FLIGHT 3 /* adsb_submit_* calls that may be pending at once */
#endif

/* Input sample formats (the `format` / `fmt` argument).  The reference's flowgraph feeds complex64 from the
 * SDR source through complex_to_mag_squared (examples/adsb_rx.py:116,180); the integer formats are the same
 * samples as the SDR hardware delivers them, converted exactly on the device. */
#define ADSB_FMT_FC32 0 /* interleaved float32 I,Q           8 B/sample */
#define ADSB_FMT_MAG2 1 /* float32 |IQ|^2 (the framer's own input type, framer.py:38)  4 B/sample */
#define ADSB_FMT_SC16 2 /* interleaved int16 I,Q             4 B/sample   component = f32(i16) * scale   (default 1/32768) */
#define ADSB_FMT_SC8 3  /* interleaved int8 I,Q              2 B/sample   component = f32(i8) * scale    (default 1/128) */
#define ADSB_FMT_CU8 4  /* interleaved uint8 I,Q, offset binary (RTL-SDR)  2 B/sample
                         * component = f32(2*u8 - 255) * scale, i.e. (u8 - 127.5) * 2*scale, exact (default 1/255).
                         * A power-of-two scale -- e.g. 2^-8: the (u8 - 127.5) / 128 of the usual RTL-SDR front ends -- runs, like a
                         * power-of-two int8 scale, an instance of the streaming kernel that squares with integer dot products:
                         * same bits, 4-6 % faster */
#define ADSB_FMT_COUNT 5

/* adsb_create flags */
#define ADSB_FLAG_TIMING 1u /* bracket the detect kernel with HIP events (adsb_get_stats) */
/* Opt-in extension, NOT the reference's behaviour: the re-trigger gate holds for the length of the
 * burst it accepted -- 119*sps when the burst's first data bit is set (DF >= 16: a 112-bit reply), 63*sps otherwise --
 * instead of always assuming a short reply (framer.py:163-165), so the second half of a long reply can no longer
 * raise false tags.  Applies to adsb_process_* / adsb_submit_* / adsb_shard_*; adsb_framer_work (the exact GNU Radio
 * emulation) ignores it.  Records of such a context carry ADSB_BURST_LONG_HINT, which adsb_shard_fixup / adsb_stitch
 * honour. */
#define ADSB_FLAG_LONG_AWARE_GATE 2u
/* Opt-in: keep what demod.work() keeps as self.bit_confidence (demod.py:97-101, never published by the reference) for
 * every delivered burst of the whole-buffer entry points -- the float32 ratios bit1_amp / bit0_amp, see
 * adsb_last_confidence.  Costs one extra small kernel and copy per call. */
#define ADSB_FLAG_CONFIDENCE 4u
/* Run the sparse tail of a pass on the compute stream behind its k_detect instead of on a second stream beside the
 * next pass's k_detect (profiling aid: serial kernels; about 15 % less throughput with several calls in flight). */
#define ADSB_FLAG_SINGLE_STREAM 8u
/* Pipelined use (adsb_submit_*): let the sparse tail of a pass (ordering, gate, compaction of the burst records) run on
 * the GPU BESIDE the next pass's streaming kernel instead of after it: results arrive about one pass earlier and two
 * calls in flight suffice, for 1-2 % less throughput.  Default off = maximum throughput. */
#define ADSB_FLAG_LOW_LATENCY 16u
/* adsb_framer_work also slices the 112 bits of every tag whose burst ends inside the call's input
 * (offset + 119*sps + sps/2 < nitems_written + N, the rule of demod.py:82 applied to the framer's own chunk): such tags
 * come back with ADSB_BURST_DEMOD, bits and the parity pre-filter flags -- the one device pass a framer/demod pair of
 * one flowgraph needs (gr_adsb_amd.blocks.demod(fs, framer=...)); default off: tags carry offset / peak / median only. */
#define ADSB_FLAG_FRAMER_SLICES 32u
/* Host-side NUMA placement is ON by default: the context looks up the NUMA node and the cpus local to its GPU's PCI device
 * (/sys/bus/pci/devices/<bdf>/numa_node, local_cpulist), allocates its page-locked buffers (staging ring, result and
 * summary buffers) on that node and runs its copy threads on those cpus -- on a two-socket 8-GPU node (one process per GPU,
 * SURVEY.md §8e) half of the host-fed traffic would otherwise cross the socket interconnect.  This flag turns it off
 * (adsb_numa_info still reports what was found).  No reference counterpart: the reference is one Python thread. */
#define ADSB_FLAG_NO_NUMA_BINDING 64u
/* Opt-in: the decoder's error_corr="Conservative" (decoder.py:738-780) on the device.  Every delivered record with
 * ADSB_BURST_DEMOD whose DF is 11/17/18/19 and whose syndrome is non-zero is looked up in the decoder's table of 1-bit and
 * 2-adjacent-bit error patterns (adsb_mode_s_fec states the rule): a repair that keeps a DF of that set and its length is
 * applied to bits[] (ADSB_BURST_FEC_FIXED, the pre-filter bits then describe the repaired reply); a repair that would change
 * the format leaves the bits raw (ADSB_BURST_FEC_DF).  One small kernel per pass, queued before the records reach the host;
 * every entry point that returns records applies it, and adsb_demod_work applies it to its slices.  Without the flag nothing
 * is launched and no byte changes.  Confidence ratios stay those of the raw slice (demod.py:101). */
#define ADSB_FLAG_FEC_CONSERVATIVE 128u
/* Opt-in: the decoder's aircraft table (plane_dict, decoder.py:576-665) on the device, so that address/parity (AP) replies --
 * DF 0/4/5/16/20/21/24, accepted by the decoder only when AA = crc(bits[0:L-24]) ^ bits[L-24:L] is an address it has heard --
 * get a verdict too.  The table models one decoder (msg_filter="All Messages", error_corr "None", or "Conservative" with
 * ADSB_FLAG_FEC_CONSERVATIVE) that consumes the context's published PDUs in publication order: call order, adsb_submit_*
 * in submission order (not wait order), within a call the delivered records with ADSB_BURST_DEMOD (adsb_demod_work: the
 * slices with ok != 0) in order.  Every such record that the decoder would accept and that reaches update_plane announces
 * its address (adsb_mode_s_aircraft states the per-PDU rule); an AP reply is flagged ADSB_BURST_AP_KNOWN when its AA was
 * announced earlier.  The table lives as long as the context (128 MiB of device memory, allocated only with the flag):
 * adsb_reset clears it; addresses never time out, as in the decoder (unless the caller expires them: PLANE AGES).  Applies to adsb_process_*, adsb_submit_* and
 * adsb_demod_work; adsb_framer_work ignores it (its records are not what is published); the sharded entry points
 * (adsb_shard_*, adsb_submit_shard_device, adsb_process_sharded_*) return -EINVAL: their stitch decides publication after
 * the device has run.  Without the flag nothing is allocated or launched and no byte changes. */
#define ADSB_FLAG_AIRCRAFT_TABLE 256u
/* Opt-in, requires ADSB_FLAG_AIRCRAFT_TABLE (adsb_create: -EINVAL without it): the rest of the decoder on the device --
 * decode_message / decode_me (decoder.py:883-1301: callsigns, AC13 / AC12 altitudes, velocities, the CPR global decode of
 * :1309-1512), update_plane and the published ports (:413-440, :512-538) -- for the same PDUs, in the same publication order
 * as the table, as one decoder with msg_filter set by adsb_set_decoder (default "All Messages") and error_corr
 * "Conservative" iff ADSB_FLAG_FEC_CONSERVATIVE, else "None".  Every delivered record gets an adsb_decoded row
 * (adsb_last_decoded); adsb_decode_pdus decodes already-published PDUs through the same state.
 * The decoder's clock is the PDU's own timestamp: now = int(timestamp) (Python truncation), the timestamp of a record
 * being start_timestamp + offset / fs in float64 (blocks.make_pdu) -- what the reference computes with int(time.time()) when it
 * decodes in real time with zero latency.  CPR frames age out after 30 s of that clock; nothing else times out.
 * State: one 88-byte entry per 24-bit address (2^24 entries, 1.375 GiB of device memory, allocated only with the flag),
 * valid when its epoch is the context's: adsb_reset clears every plane in O(1).  The key "" that the decoder files a few
 * PDUs under (a reply whose repair made it an address/parity format) is not an address: such PDUs touch no plane.
 * adsb_framer_work, adsb_demod_work and the sharded entry points return -EINVAL.  Without the flag nothing is allocated or
 * launched. */
#define ADSB_FLAG_DECODE 512u
/* Opt-in, for receiver streams (adsb_streams_open): ONE DECODER BEHIND EVERY STREAM, the reference's topology of one decoder
 * block behind each receiver's demod (examples/adsb_rx.py, decoder.py:325-352), for the whole fleet in one device step per
 * adsb_process_stream_batch* call -- see STREAM DECODERS below.  -EINVAL together with ADSB_FLAG_AIRCRAFT_TABLE, _DECODE or
 * _CONFIDENCE; combines with ADSB_FLAG_FEC_CONSERVATIVE (error_corr "Conservative", else "None") and
 * ADSB_FLAG_LONG_AWARE_GATE.  Nothing is allocated at create; every entry point other than the stream ones behaves as on a
 * context without the flag (adsb_last_decoded, adsb_decode_pdus and adsb_set_decoder: -EINVAL).  Without the flag nothing
 * is allocated or launched and no byte changes. */
#define ADSB_FLAG_STREAM_DECODE 1024u
/* Opt-in, only together with ADSB_FLAG_DECODE or ADSB_FLAG_STREAM_DECODE (adsb_create: -EINVAL otherwise): the decoders keep
 * plane_dict's last_seen on the device, so that planes can be read back with their age and expired by it -- see PLANE AGES
 * below.  One int64 per address beside the planes of one decoder (2^24 entries, 128 MiB), one per slot beside a fleet's
 * store.  Without the flag nothing is allocated or launched and no byte changes. */
#define ADSB_FLAG_PLANE_AGES 2048u
/* Opt-in, only together with ADSB_FLAG_STREAM_DECODE (adsb_create: -EINVAL otherwise): ONE DECODER BEHIND ALL STREAMS, the
 * reference's fan-in of several demod blocks into one decoder block (decoder.py:325-352: one plane_dict, fed in arrival
 * order) -- see SHARED DECODER below.  Every delivered adsb_process_stream_batch* call publishes its records to that one
 * decoder in time order, so an aircraft whose replies are split over receivers is decoded as one receiver that heard them all
 * would decode it.  Combines with ADSB_FLAG_FEC_CONSERVATIVE, _LONG_AWARE_GATE and _PLANE_AGES exactly as
 * ADSB_FLAG_STREAM_DECODE does.  Without the flag nothing is allocated or launched and no byte of any existing call changes. */
#define ADSB_FLAG_STREAM_DECODE_SHARED 4096u
/* Shared decoders only (valid together with ADSB_FLAG_STREAM_DECODE | ADSB_FLAG_STREAM_DECODE_SHARED, adsb_create returns
 * -EINVAL otherwise): a reply heard by several receivers is published once -- see DE-DUPLICATION below.  Without the flag
 * nothing is allocated or launched and no byte of any call changes. */
#define ADSB_FLAG_STREAM_DEDUP 8192u
/* Opt-in: soft-decision CRC repair of weak-bit errors -- see SOFT REPAIR below.  A DF 11/17/18/19 reply that failed parity and
 * that the Conservative table does not explain is repaired from the confidence of its own bits: the subset of its n_weak
 * weakest bits whose syndromes add up to the reply's.  No reference counterpart: error_corr "Brute Force" only logs "to be
 * implemented" (decoder.py:772-776), and the reference's decoder never sees the samples.  One small kernel per pass behind the
 * Conservative repair's, before the table and decode steps, which then see a repaired reply as one that passed parity.
 * Combines with ADSB_FLAG_FEC_CONSERVATIVE, _LONG_AWARE_GATE, _AIRCRAFT_TABLE, _DECODE, _PLANE_AGES, _CONFIDENCE (the ratios stay
 * those of the raw slice) and _TIMING; adsb_create returns -EINVAL with ADSB_FLAG_STREAM_DECODE or ADSB_FLAG_FRAMER_SLICES, and
 * the batch, stream-batch and sharded entry points refuse such a context as they refuse ADSB_FLAG_CONFIDENCE contexts.  Without
 * the flag nothing is allocated or launched and no byte of any call changes. */
#define ADSB_FLAG_FEC_SOFT 16384u
/* Opt-in: the same soft-decision repair for MANY receivers -- see SOFT REPAIR, IN A BATCH below.  adsb_process_batch* and
 * adsb_process_stream_batch* repair the packed record list of the pass against each record's OWN item's samples (one more small
 * kernel behind the Conservative repair's), so a reply that one distant receiver heard with a few weak wrong bits reaches the
 * shared decoder, the de-duplication and the multilateration with the payload the other receivers heard.  The rows come back
 * through adsb_batch_last_soft; the rule is adsb_set_soft_fec's.  Combines with ADSB_FLAG_FEC_CONSERVATIVE, _LONG_AWARE_GATE,
 * _TIMING and _STREAM_DECODE (with _SHARED, _DEDUP, _PLANE_AGES).  adsb_create returns -EINVAL with ADSB_FLAG_FEC_SOFT (one
 * meaning per context) and with ADSB_FLAG_CONFIDENCE, _AIRCRAFT_TABLE, _DECODE or _FRAMER_SLICES (the batch entry points refuse
 * those contexts anyway).  The context's other entry points return exactly what they return without the flag; the sharded
 * drivers do not repair.  Without the flag nothing is allocated or launched and no byte of any call changes. */
#define ADSB_FLAG_FEC_SOFT_BATCH 32768u

/* adsb_burst.flags */
#define ADSB_BURST_DEMOD 1u /* eob inside the demod input: bits[] valid, a PDU is published (demod.py:82) */
#define ADSB_BURST_KEPT 2u  /* passed the framer's re-trigger gate (framer.py:121) */
#define ADSB_BURST_HEAD 16u /* shard mode: part of the shard's head region (see adsb_shard_device) */
/* Mode S parity pre-filter, computed on the device for every burst with ADSB_BURST_DEMOD:
 * what the decoder's first two steps (decoder.py:550-556 decode_header, :560-688 check_parity) will find,
 * so a consumer can drop garbage PDUs before they reach the (scalar, per-message) decoder.  Advisory: the
 * bits and every other field are unchanged, and the reference-compatible blocks publish all PDUs. */
#define ADSB_BURST_PARITY_OK 32u /* DF 11/17/18/19 and crc(bits[0:L-24]) == bits[L-24:L] (decoder.py:625,679); the
                                    address/parity formats' verdict needs an aircraft table: ADSB_FLAG_AIRCRAFT_TABLE */
#define ADSB_BURST_LONG 64u      /* DF 16-21/24: 112-bit reply (decoder.py:636,669); else the 56-bit reading */
#define ADSB_BURST_KNOWN_DF 128u /* DF is one check_parity() handles: 0,4,5,11,16,17,18,19,20,21,24 */
#define ADSB_BURST_DF_SHIFT 8    /* (flags >> 8) & 31 = downlink format (decoder.py:551) */
#define ADSB_BURST_DF(flags) (((flags) >> ADSB_BURST_DF_SHIFT) & 31u)
#define ADSB_BURST_LONG_HINT 0x2000u /* long-aware contexts only: this burst holds the gate for 119*sps */
/* ADSB_FLAG_FEC_CONSERVATIVE contexts only (kDemod records of DF 11/17/18/19 that failed parity): */
#define ADSB_BURST_FEC_FIXED 0x4000u /* a 1-bit / 2-adjacent-bit error was repaired: bits[] and the pre-filter bits are the repaired reply's */
#define ADSB_BURST_FEC_DF 0x8000u    /* the decoder's repair would change the DF (or its length): bits[] left raw */
/* ADSB_FLAG_AIRCRAFT_TABLE contexts only (ADSB_BURST_DEMOD records of DF 0/4/5/16/20/21/24); the two values are never
 * set on a delivered record otherwise.  adsb_demod_work's ok[]: bit 3 (8) = AP_KNOWN, bit 4 (16) = AP_FEC. */
#define ADSB_BURST_AP_FEC 0x0004u    /* with ADSB_FLAG_FEC_CONSERVATIVE: AA unknown, but the decoder's repair accepts the reply (bits[] stay raw) */
#define ADSB_BURST_AP_KNOWN 0x0008u  /* AA was announced by an earlier published reply: the decoder accepts it */

typedef struct adsb_ctx adsb_ctx;

/* One detected burst == one "burst" stream tag (framer.py:168-174) plus, when ADSB_BURST_DEMOD is set,
 * the payload of the PDU demod would publish for it (demod.py:104-110).  32 bytes, little endian. */
typedef struct adsb_burst {
  int64_t offset;   /* absolute stream offset of the tag: centre of the first preamble pulse */
  float peak;       /* in0[pulse_idx]                       (framer.py:157) */
  float median;     /* np.median of the <=100 samples before (framer.py:157-159) */
  uint8_t bits[14]; /* 112 hard bits, first bit = MSB of bits[0] (demod.py:94-95) */
  uint16_t flags;
} adsb_burst;

/* ADSB_FLAG_DECODE: what the decoder made of one delivered record (adsb_last_decoded, adsb_decode_pdus).  72 bytes. */
#define ADSB_DEC_NONE 0u      /* nothing published */
#define ADSB_DEC_DECODED 1u   /* published on "decoded" (decoder.py:512-526): the plane's fields below */
#define ADSB_DEC_UNKNOWN 2u   /* published on "unknown" (:529-538) */
#define ADSB_DEC_RAISED 3u    /* decode_packet raises before it publishes: DF 18 CF 2/3/5, TC 19 ST 0/5/6/7 */
#define ADSB_DEC_DUPLICATE 4u /* ADSB_FLAG_STREAM_DEDUP: another receiver's hearing of this reply was published; this one was not */
#define ADSB_DEC_HAS_PLANE 1u     /* plane_dict[icao] exists after the PDU: the fields below are its snapshot */
#define ADSB_DEC_HAS_CALLSIGN 2u  /* callsign is not None */
#define ADSB_DEC_HAS_ALTITUDE 4u  /* altitude is not NaN */
#define ADSB_DEC_HAS_VELOCITY 8u  /* speed, heading and vertical_rate are not NaN */
#define ADSB_DEC_ALL_MESSAGES 0          /* adsb_set_decoder msg_filter values */
#define ADSB_DEC_EXTENDED_SQUITTER_ONLY 1
typedef struct adsb_decoded {
  uint8_t port;          /* ADSB_DEC_* */
  uint8_t df;            /* self.df after the PDU (the repaired reply's when the decoder repaired it) */
  uint8_t present;       /* ADSB_DEC_HAS_* */
  uint8_t pad0;
  int32_t icao;          /* the address the PDU is filed under (self.aa_str), -1 for "" */
  uint8_t bits[14];      /* the decoder's bits after the PDU: what a published PDU carries (packed, MSB first) */
  char callsign[8];      /* NUL padded, "_" removed */
  uint8_t pad1[2];
  int32_t altitude;
  int32_t velocity_we;   /* speed = sqrt(velocity_sn^2 + velocity_we^2), heading = arctan2(velocity_sn, velocity_we)*360/(2 pi) */
  int32_t velocity_sn;
  int32_t vertical_rate;
  double latitude;       /* NaN until a fix */
  double longitude;
  uint32_t num_msgs;
  uint32_t pad2;
} adsb_decoded;

typedef struct adsb_stats {
  uint64_t detect_launches;  /* k_detect launches timed */
  double detect_ms;          /* sum of their HIP-event durations */
  uint64_t detect_samples;   /* samples those launches covered */
  uint64_t detect_bytes;     /* algorithmic bytes: samples x the format's bytes per sample */
  uint64_t calls;
  uint64_t retries;          /* record-capacity regrowths */
  uint64_t longrun_calls;    /* calls that needed the long-pulse kernel */
  uint64_t detect_grid;      /* workgroups of the last k_detect launch */
  uint64_t blocks_per_cu;    /* resident k_detect workgroups per CU (occupancy query): four wavefronts each, one for the 8-bit formats */
  double detect_gap_ms;      /* sum of idle gaps on the compute stream between consecutive timed k_detect launches */
  uint64_t detect_gaps;      /* number of gaps summed */
  uint64_t longrun_pulses;   /* pulses longer than k_detect's LDS window, handled by the long-pulse kernel (sum over calls) */
  uint64_t poll_fallbacks;   /* ABI 3: small passes whose pass number did not appear within the short spin and were waited for
                              * by blocking on the stream instead (adsb_hip.hip: finish) */
  uint64_t shard_fallbacks;  /* ABI 4: shards of adsb_process_sharded_device whose head region ended inside a chain of overlapping
                              * bursts and were run a second time (larger head, then ungated + greedy gate) */
} adsb_stats;

int adsb_abi_version(void);

/* fs must be an even multiple of 1e6 (the reference asserts fs % 1e6 == 0, framer.py:44, and only
 * works for even sps) between 2e6 and ADSB_MAX_SPS * 1e6: otherwise -EINVAL.  2 / 4 / 8 / 20 Msps run
 * kernels with the preamble tap stride (sps / 2, framer.py:137) compiled in, every other rate ("2 Msps, 4 Msps, 6 Msps,
 * etc", README.md:17) the run-time-stride instances; all are pinned by reference vectors (tests/golden/R*.npz: 6, 10, 12,
 * 16, 24, 40 and 100 Msps).  The reference itself has no upper limit; above 100 Msps nothing is tested, so nothing is
 * accepted.  device = HIP ordinal. */
int adsb_create(double fs, float threshold, int device, uint32_t flags, adsb_ctx** out);
void adsb_destroy(adsb_ctx* ctx);
int adsb_set_threshold(adsb_ctx* ctx, float threshold);
/* Use an existing hipStream_t (e.g. torch's current stream) instead of the context's own compute stream: device
 * input produced by work queued on that stream needs no host synchronisation before adsb_process_*_device /
 * adsb_submit_*.  With the context's own stream (the default) the caller synchronises producers of a device
 * buffer first.  -EBUSY while submitted calls are pending.  A context is used from one thread at a time;
 * different contexts are independent. */
int adsb_set_stream(adsb_ctx* ctx, void* hip_stream);
/* Host threads (1..64, the caller included) that copy PAGEABLE sources of adsb_submit_format_host into the pinned staging
 * ring; default 6 on hosts with >= 16 cpus.  Before the first pageable submission only (-EBUSY afterwards).  Page-locked
 * sources (adsb_host_alloc, adsb_host_register) never touch these threads: they are DMA'd where they lie. */
int adsb_set_copy_threads(adsb_ctx* ctx, int32_t threads);
/* memcpy split over the context's copy threads (the GNU Radio passthrough `out0[:] = in0` of multi-megabyte chunks:
 * framer.py:181, demod.py:135).  Plain host memory on both sides; blocking. */
int adsb_host_copy(adsb_ctx* ctx, void* dst, const void* src, size_t bytes);
/* Order the NEXT call on this context -- blocking, adsb_submit_* or the sharded driver's first pass -- AFTER a HIP event of the
 * caller (hipEvent_t recorded on the stream that produces a device-resident input, e.g. a framework's current stream): a
 * device-side dependency, the host does not wait.  ABI 4: submitted passes run on one stream per pipeline slot, so the wait is
 * queued with that next call, on the stream its first operation runs on (a host-fed submission: the upload stream); a later submission that depends on the same producer asks again.  Up to four events may be pending.  The
 * event must stay alive until that next call has returned. */
int adsb_wait_for_event(adsb_ctx* ctx, void* hip_event);
/* Pending events are consumed by the next call that queues GPU work.  A call that returns before it queues anything (an
 * argument error, -EBUSY, n == 0, adsb_demod_work without tags) leaves them pending for the call after it -- the events must
 * stay alive until then, or be dropped with adsb_clear_pending_events (ABI 5; adsb_reset drops them too). */
int adsb_clear_pending_events(adsb_ctx* ctx);
/* Forget the framer's cross-call state (prev_in0 = 0, prev_eob = -1; framer.py:54,57) and any pending adsb_wait_for_event. */
int adsb_reset(adsb_ctx* ctx);
/* The framer's two words of cross-call state as the reference keeps them on the block (framer.py:54 `prev_in0`, :57
 * `prev_eob_idx`, both public attributes there): what adsb_framer_work carries between calls.  Either pointer may be NULL. */
int adsb_framer_state(adsb_ctx* ctx, float* prev_in0, int64_t* prev_eob_idx);

/* Canonical whole-buffer mode: ONE framer.work() call over n samples of a fresh stream (history =
 * 8*sps-1 zeros) followed by ONE demod.work() call over the same n samples with all tags delivered.
 * iq: n interleaved complex64 (2n floats).  abs_offset: stream offset of sample 0.  Output: the
 * kept bursts in stream order; bursts whose eob falls outside the buffer have ADSB_BURST_DEMOD clear
 * (tag emitted, PDU dropped: demod.py:130-133).  Stateless across calls. */
int adsb_process_iq(adsb_ctx* ctx, const float* iq_host, int64_t n, int64_t abs_offset,
                    adsb_burst* out, int32_t cap, int32_t* n_out);
int adsb_process_mag2(adsb_ctx* ctx, const float* mag2_host, int64_t n, int64_t abs_offset,
                      adsb_burst* out, int32_t cap, int32_t* n_out);
/* Page-locked host memory for IQ buffers handed to adsb_process_iq / adsb_process_mag2 / adsb_framer_work:
 * buffers allocated here (or any other pinned host memory) are DMA'd straight to the device; pageable
 * buffers are first copied into the context's own pinned staging buffer (about 3x slower end to end). */
int adsb_host_alloc(void** p, size_t bytes);
int adsb_host_free(void* p);
/* The same on the NUMA node of the context's GPU (see ADSB_FLAG_NO_NUMA_BINDING): what a feeder should fill its IQ ring
 * from, so that the H2D DMA reads local memory.  Freed with adsb_host_free. */
int adsb_host_alloc_near(adsb_ctx* ctx, void** p, size_t bytes);
/* Where the context's host side lives: NUMA node of the GPU's PCI device (-1: unknown / not bound), the cpus local to it
 * as sysfs prints them ("0-63,128-191", "" if unknown) and the device's PCI address ("0000:c1:00.0").  Any pointer may be
 * null.  For reports (bench.py prints it per rank) and for callers that want to pin their own feeder threads. */
int adsb_numa_info(adsb_ctx* ctx, int32_t* node, char* cpulist, size_t cpulist_cap, char* pci_bdf, size_t bdf_cap);
/* Page-lock a buffer the caller already owns (e.g. the ring an SDR driver or a file mapping fills), so that
 * adsb_process_* / adsb_submit_format_host DMA it where it lies instead of copying it through the context's staging
 * chunks (about half the rate).  Registration costs milliseconds: do it once per buffer, not per call; unregister before
 * freeing the memory.  Thin wrappers over hipHostRegister / hipHostUnregister for callers that do not link HIP. */
int adsb_host_register(void* p, size_t bytes);
int adsb_host_unregister(void* p);

/* Same, input already in HBM (16-byte aligned device pointer).  out may be NULL: the result stays in
 * the context's pinned buffer, see adsb_last_result. */
int adsb_process_iq_device(adsb_ctx* ctx, const void* d_iq, int64_t n, int64_t abs_offset,
                           adsb_burst* out, int32_t cap, int32_t* n_out);
int adsb_process_mag2_device(adsb_ctx* ctx, const void* d_mag2, int64_t n, int64_t abs_offset,
                             adsb_burst* out, int32_t cap, int32_t* n_out);
/* int16 IQ (interleaved I,Q shorts, 4 B/sample: the SDR's native wire format).  Each
 * component becomes float32 exactly and is multiplied by `scale` (float32, one rounded multiply; default
 * 1/32768) before |IQ|^2; everything downstream is identical to the complex64 path. */
int adsb_set_iq16_scale(adsb_ctx* ctx, float scale);
int adsb_process_iq16(adsb_ctx* ctx, const int16_t* iq16_host, int64_t n, int64_t abs_offset,
                      adsb_burst* out, int32_t cap, int32_t* n_out);
int adsb_process_iq16_device(adsb_ctx* ctx, const void* d_iq16, int64_t n, int64_t abs_offset,
                             adsb_burst* out, int32_t cap, int32_t* n_out);
/* Any format by number (ADSB_FMT_*): the entry points above are adsb_process_format[_device] with format 0, 1, 2.
 * Integer components become float32 exactly and are multiplied by the format's scale (one rounded float32
 * multiply) before |IQ|^2 = re*re + im*im with separately rounded products; downstream is identical.
 * adsb_set_format_scale: format must be one of the integer formats (-EINVAL otherwise). */
int adsb_set_format_scale(adsb_ctx* ctx, int format, float scale);
int adsb_process_format(adsb_ctx* ctx, int format, const void* host, int64_t n, int64_t abs_offset,
                        adsb_burst* out, int32_t cap, int32_t* n_out);
int adsb_process_format_device(adsb_ctx* ctx, int format, const void* d_data, int64_t n, int64_t abs_offset,
                               adsb_burst* out, int32_t cap, int32_t* n_out);
int adsb_last_result(adsb_ctx* ctx, const adsb_burst** bursts, int32_t* n);
/* ADSB_FLAG_CONFIDENCE contexts: *ratio -> n x 112 float32 in the context's pinned memory, row t = bit1_amp / bit0_amp
 * of burst t of the last finished call (demod.py:91-101: 10*log10 of it is bit_confidence; +-inf / NaN where the
 * reference has them); rows of bursts without ADSB_BURST_DEMOD are zero.  Valid until the same pipeline slot is
 * used again.  -EINVAL on a context created without the flag. */
int adsb_last_confidence(adsb_ctx* ctx, const float** ratio, int32_t* n);
/* ADSB_FLAG_DECODE contexts: the decoder's msg_filter (ADSB_DEC_ALL_MESSAGES / _EXTENDED_SQUITTER_ONLY) and the
 * start_timestamp of the records' PDU timestamps (start + offset / fs), for the calls that follow.  -EBUSY while a submitted
 * call is pending. */
int adsb_set_decoder(adsb_ctx* ctx, int32_t msg_filter, double start_timestamp);
/* ADSB_FLAG_DECODE contexts: *rows -> n adsb_decoded in the context's pinned memory, row t for record t of the last finished
 * adsb_process_* call or waited ticket.  Valid until the same pipeline slot is used again. */
int adsb_last_decoded(adsb_ctx* ctx, const adsb_decoded** rows, int32_t* n);
/* ADSB_FLAG_DECODE contexts: decode n already-published PDUs (bits14: n x 14 packed bytes; timestamps: n float64) in one
 * device call, through the context's decoder state, in call order with its other calls: parity flags, the Conservative
 * repair (with ADSB_FLAG_FEC_CONSERVATIVE), the table step and the decode step.  rows: n adsb_decoded. */
int adsb_decode_pdus(adsb_ctx* ctx, const uint8_t* bits14, const double* timestamps, int32_t n, adsb_decoded* rows);

/* Asynchronous form of adsb_process_*_device: submit queues the whole device pipeline on the context's
 * streams and returns a ticket (0 .. ADSB_MAX_IN_FLIGHT-1) at once; adsb_wait blocks for that call, copies
 * its bursts to pinned host memory on a copy stream and delivers them like adsb_process_*.  With later
 * calls submitted before waiting for call i, the streaming kernel of call i+1 runs back to back with that
 * of call i while call i's tail kernels, its PCIe copy and all host work proceed beside it.  The input
 * buffer must stay valid and unchanged until adsb_wait returns.  At most ADSB_MAX_IN_FLIGHT calls pending
 * (-EBUSY otherwise); results must be collected in submission order. */
int adsb_submit_iq_device(adsb_ctx* ctx, const void* d_iq, int64_t n, int64_t abs_offset, int32_t* ticket);
int adsb_submit_mag2_device(adsb_ctx* ctx, const void* d_mag2, int64_t n, int64_t abs_offset, int32_t* ticket);
int adsb_submit_iq16_device(adsb_ctx* ctx, const void* d_iq16, int64_t n, int64_t abs_offset, int32_t* ticket);
int adsb_submit_format_device(adsb_ctx* ctx, int format, const void* d_data, int64_t n, int64_t abs_offset, int32_t* ticket);
/* Host-fed streaming, the topology of examples/adsb_rx.py:113-126,180-196 (SDR source -> ... -> framer -> demod) with
 * the chunks in host memory: the samples are uploaded on a dedicated stream into the ticket's own device buffer, so
 * with several calls in flight the upload of chunk i+1 runs beside the kernels of chunk i and the record download of
 * chunk i-1 (PCIe both ways, compute in between).  A page-locked source (adsb_host_alloc) is DMA'd where it lies and
 * must stay valid until adsb_wait returns; a pageable source is copied through pinned chunks before the call returns
 * (the call then takes as long as that copy).  Results exactly as adsb_process_format. */
int adsb_submit_format_host(adsb_ctx* ctx, int format, const void* host, int64_t n, int64_t abs_offset, int32_t* ticket);
int adsb_submit_shard_device(adsb_ctx* ctx, int fmt, const void* d_data, int64_t n, int64_t origin, int64_t own_lo,
                             int64_t own_hi, int64_t stream_len, int32_t head_cands, int32_t* ticket);
int adsb_wait(adsb_ctx* ctx, int32_t ticket, adsb_burst* out, int32_t cap, int32_t* n_out);

/* GNU Radio sync-block emulation, framer.work(): in0 holds N + 8*sps - 1 floats of |IQ|^2 (history
 * first), exactly what the scheduler hands the Python block; nitems_written = nitems_written(0).
 * Emits the tags of this call (offset/peak/median; flags = KEPT) and carries prev_in0 / prev_eob_idx
 * inside ctx exactly like the reference (including its stale-state behaviour, framer.py:177-179). */
int adsb_framer_work(adsb_ctx* ctx, const float* in0, int64_t n_in0, int64_t N, int64_t nitems_written,
                     adsb_burst* tags, int32_t cap, int32_t* n_out);
/* The same plus the block's pass-through (framer.py:181 `out0[:] = in0[history:]`): out0 (N floats, may be NULL) is filled
 * on the host WHILE the device pass runs -- the copy of a multi-megabyte chunk no longer stands behind the pass (ABI 5). */
int adsb_framer_work_passthrough(adsb_ctx* ctx, const float* in0, int64_t n_in0, int64_t N, int64_t nitems_written, float* out0,
                                 adsb_burst* tags, int32_t cap, int32_t* n_out);

/* demod.work(): in0 = this call's n input floats, nitems_read = nitems_read(0) (== nitems_written(0)
 * for a sync block); tag_offsets = absolute offsets of the "burst" tags inside [nitems_read,
 * nitems_read+n).  bits112: ntags*112 bytes of 0/1 (the u8vector the PDU carries); ok[t] != 0 when the
 * burst was demodulated, 0 when it straddles the end of the chunk and is dropped (demod.py:82,130-133);
 * a non-zero ok[t] is ADSB_BURST_DEMOD | the pre-filter bits ADSB_BURST_PARITY_OK / _LONG / _KNOWN_DF, and on an
 * ADSB_FLAG_FEC_CONSERVATIVE context ADSB_BURST_FEC_FIXED >> 13 (2) / ADSB_BURST_FEC_DF >> 13 (4), with bits112 repaired; on an
 * ADSB_FLAG_AIRCRAFT_TABLE context ADSB_BURST_AP_KNOWN (8) / ADSB_BURST_AP_FEC << 2 (16), the slices with ok != 0 being
 * the call's published PDUs, in tag order.
 * ratio (optional, may be NULL): ntags*112 floats bit1_amp/bit0_amp; 10*log10 of it is
 * demod.bit_confidence (demod.py:101). */
int adsb_demod_work(adsb_ctx* ctx, const float* in0, int64_t n, int64_t nitems_read,
                    const int64_t* tag_offsets, int32_t ntags, uint8_t* bits112, uint8_t* ok, float* ratio);

/* Overlapped time shards (multi-GPU): the device buffer holds stream samples [origin, origin+n) of
 * which this shard owns the pulse rises in [own_lo, own_hi) (stream offsets).  stream_len = length of
 * the whole stream (for the end-of-stream rules); fmt = ADSB_FMT_*.
 *   head_cands == 0: returns EVERY matched preamble centre of the owned range, not gated (KEPT never
 *     set); adsb_stitch applies the gate over the concatenation of all shards.
 *   head_cands  > 0: the gate runs on the device as if the shard started a fresh stream (KEPT set), and
 *     the first head_cands centres of the shard are returned whether gated or not (HEAD set): with the
 *     previous shard's end-of-burst state adsb_shard_fixup then makes the result exact on the host, so
 *     ranks exchange 8 bytes instead of candidate lists.
 * -EOVERFLOW when a pulse or burst runs past the shard's halo. */
int adsb_shard_device(adsb_ctx* ctx, int fmt, const void* d_data, int64_t n, int64_t origin,
                      int64_t own_lo, int64_t own_hi, int64_t stream_len, int32_t head_cands,
                      adsb_burst* out, int32_t cap, int32_t* n_out);
/* The same from a host buffer (uploaded like adsb_process_*): for callers that receive the stream block by block
 * in host memory -- the chunk-invariant ("improved") GNU Radio blocks and file replay without torch.  origin may
 * be negative when the buffer starts with the zero history in front of a fresh stream.
 * shard_flags: ADSB_SHARD_DROP_OVERLONG = a pulse still high at the end of the buffer is left out of the result
 * (as framer.py:102-108 leaves out a pulse still high at the end of a call) instead of failing with -EOVERFLOW. */
#define ADSB_SHARD_DROP_OVERLONG 1u
int adsb_shard_host(adsb_ctx* ctx, int fmt, const void* host, int64_t n, int64_t origin, int64_t own_lo,
                    int64_t own_hi, int64_t stream_len, int32_t head_cands, uint32_t shard_flags,
                    adsb_burst* out, int32_t cap, int32_t* n_out);
/* The tiling every sharded caller uses (gr_adsb_amd/frontend.py: shard_plan; bench.py's ranks; file replay; the driver
 * below): shard g of n_shards over a stream of stream_len samples owns the pulse rises of [*own_lo, *own_hi) -- equal
 * ranges of a multiple of `align` samples -- and needs the samples [*lo, *hi): 100 + 8*sps + 4 of back halo (noise window,
 * framer.py:31,156; preamble span), *lo on a 16-byte boundary of every format, and 256 + 121*sps of forward halo (the longest
 * pulse followed, preamble + 112 bits: framer.py:165, demod.py:76).  Pure host arithmetic; 0 or -EINVAL. */
int32_t adsb_shard_bounds(int64_t stream_len, int32_t n_shards, int32_t g, int sps, int64_t align, int64_t* own_lo,
                          int64_t* own_hi, int64_t* lo, int64_t* hi);
/* ONE resident stream processed as `shards` overlapped time shards on THIS device -- BASELINE config 4's decomposition
 * (one 20 Msps stream tiled as N overlapped shards) run where there is one GPU, or many receivers' worth of mid-size
 * buffers multiplexed on it: the shards are planned (adsb_shard_bounds, align 4096), kept ADSB_MAX_IN_FLIGHT deep in the
 * pipeline, each detected and gated on the device as a fresh stream; the head of every shard is re-gated on the host with
 * the end-of-burst state carried from the shard in front of it (adsb_shard_fixup; a head that ends inside a chain of
 * overlapping bursts: the shard once more with the largest head, then ungated with the plain greedy gate).  The whole loop
 * is host C: no interpreter between two passes.  Result: bit-identical to adsb_process_format_device over the whole
 * buffer (records, order, flags except ADSB_BURST_HEAD, which is cleared).  out must hold the result (-ENOSPC with *n_out =
 * the number needed otherwise).  Replaces: one framer.work() + demod.work() over the stream (framer.py:72-182,
 * demod.py:57-136), like adsb_process_format_device; the tiling itself has no reference counterpart. */
int adsb_process_sharded_device(adsb_ctx* ctx, int format, const void* d_data, int64_t n, int64_t abs_offset,
                                int32_t shards, adsb_burst* out, int32_t cap, int32_t* n_out);
/* (d_data: memory the DEVICE can read -- device memory, e.g. adsb_device_alloc below, or page-locked host memory, which the
 * kernels then read over PCIe.  Every shard pass waits for the events of adsb_wait_for_event.  -EINVAL on an
 * ADSB_FLAG_CONFIDENCE context: the rows of adsb_last_confidence belong to the records of one pass.) */

/* ONE process, N devices, ONE host ring (ABI 5): the reference is a single process with a single IQ source
 * (examples/adsb_rx.py:242-268); this is that process with N GPUs behind it.  `host` holds n samples of `format` (page-locked
 * -- adsb_host_alloc[_near], adsb_host_register: DMA'd where they lie -- or pageable: through each context's staging ring);
 * ctxs[0..n_ctx) are contexts of the SAME rate, threshold, gate flag and format scale, normally one per device (several on
 * one device are allowed: that is how a one-GPU box tests it).  The stream is tiled into n_ctx * shards_per_ctx overlapped
 * time shards (adsb_shard_bounds, align 4096); context k takes shards [k*shards_per_ctx, (k+1)*shards_per_ctx).  Inside the
 * call one feeder thread per context -- on the cpus local to its GPU, within the process's own mask -- uploads shard i+1
 * beside the shard pass of i and the record download of i-1 (ADSB_MAX_IN_FLIGHT deep); the calling thread takes finished
 * shards in stream order, re-gates every head with the end-of-burst state carried over the seam (adsb_shard_fixup) and
 * appends the kept records to `out`; a head that ends inside a chain of overlapping bursts has its shard run again on its
 * own context (head 4096, then ungated + the plain greedy gate: exact in every case).  No collective, no second process:
 * one int64 crosses each seam, on the host.  Result: bit-identical to adsb_process_format over the whole buffer (records,
 * order, flags except ADSB_BURST_HEAD, cleared).  -ENOSPC with *n_out = the number needed when `out` is too small; on any
 * other error nothing stays in flight on any context and adsb_last_error(ctxs[0]) names the cause.  stats may be NULL. */
#define ADSB_MULTI_MAX_CTX 64
typedef struct adsb_multi_stats {
  int32_t contexts, shards, fallbacks, pad_;
  double wall_s;                         /* the whole call */
  double feeder_s[ADSB_MULTI_MAX_CTX];   /* context k's feeder thread: first upload queued -> last shard collected */
  int32_t device[ADSB_MULTI_MAX_CTX];    /* HIP ordinal of context k */
  int32_t numa_node[ADSB_MULTI_MAX_CTX]; /* NUMA node its pinned buffers and feeder live on (-1: unknown / not bound) */
} adsb_multi_stats;
int adsb_process_sharded_multi(adsb_ctx* const* ctxs, int32_t n_ctx, int format, const void* host, int64_t n,
                               int64_t abs_offset, int32_t shards_per_ctx, adsb_burst* out, int32_t cap, int32_t* n_out,
                               adsb_multi_stats* stats);
/* MANY receivers, ONE device pass: a batch of n_items INDEPENDENT streams ("items") of one format on one context (one fs).
 * Every item is a fresh stream of its own -- its own zero history, noise-window clamp, prev_eob_idx = -1 and end-of-call
 * rules (framer.py:54-57,102-108, demod.py:82) -- with its own stream offset and threshold: item i's records are exactly
 * those adsb_process_format_device(ctx, format, data, n, abs_offset, ...) returns on a context whose threshold is
 * items[i].threshold -- same records, same order, same bytes -- concatenated in item order: out[item_first[i] ..
 * item_first[i+1]) belong to item i, *n_out = item_first[n_items] (item_first holds n_items + 1 entries).  One launch runs one
 * workgroup per item (k_batch) and a second packs the items' records (k_batch_pack): N receivers cost one pass, not N.
 * The format scale, fs, ADSB_FLAG_LONG_AWARE_GATE and ADSB_FLAG_FEC_CONSERVATIVE come from the context and apply to every item.
 * Items longer than ADSB_BATCH_ITEM_MAX samples, and items whose centre lists overflow the batch kernel's capacity, are run
 * through the ordinary pass inside the call and their records take the item's place (*n_fallback counts them; may be NULL):
 * the result never depends on the batch kernel's capacity.  Few LONG items are better served by adsb_submit_format_device.
 * -ENOSPC with *n_out = the number needed when cap is too small; -EBUSY while submitted tickets are pending; -EINVAL for a
 * bad format, a pointer that is not 16-byte aligned, reserved != 0, n < 0, and on contexts with ADSB_FLAG_AIRCRAFT_TABLE,
 * ADSB_FLAG_DECODE or ADSB_FLAG_CONFIDENCE (one table, one row set, one ratio list model ONE receiver).  n_items == 0 succeeds.
 * The framer state of adsb_framer_work and the result of adsb_last_result are left alone, with or without fallback items (a
 * fallback pass runs in a pipeline slot other than the one adsb_last_result refers to; adsb_get_stats counts it in calls / retries).  Pending adsb_wait_for_event events
 * are consumed by the call's first GPU operation.  No reference counterpart: the reference is one receiver per process. */
typedef struct adsb_batch_item {
  const void* data;   /* 16-byte aligned; memory the device can read (adsb_process_batch_device) or host memory (adsb_process_batch) */
  int64_t n;          /* samples; 0 is legal and yields no records */
  int64_t abs_offset; /* stream offset of the item's sample 0 */
  float threshold;    /* this item's framer threshold: any float, <= 0 and NaN included (the reference accepts them) */
  uint32_t reserved;  /* must be 0 */
} adsb_batch_item;    /* 32 bytes */
#define ADSB_BATCH_ITEM_MAX (1ll << 22) /* longer items are legal; they take the ordinary pass inside the call */
int adsb_process_batch_device(adsb_ctx* ctx, int format, const adsb_batch_item* items, int32_t n_items, adsb_burst* out,
                              int32_t cap, int32_t* item_first, int32_t* n_out, int32_t* n_fallback);
/* The same for items in HOST memory: all items are uploaded into one device buffer of the context (page-locked sources DMA'd
 * where they lie, pageable ones through the staging ring), then run as above. */
int adsb_process_batch(adsb_ctx* ctx, int format, const adsb_batch_item* items, int32_t n_items, adsb_burst* out, int32_t cap,
                       int32_t* item_first, int32_t* n_out, int32_t* n_fallback);
/* RECEIVER STREAMS carried across batch calls.  adsb_process_batch* starts every item as a fresh stream; a receiver delivers a
 * chunk every few tens of milliseconds, indefinitely.  A context holds n_streams streams (adsb_streams_open), each with the
 * number of samples consumed (pos), a carried end-of-burst offset (eob), a base offset that its records' offsets add to the
 * stream's sample index, and -- on the device, in the wire format -- a carry of its last 100 + 8*sps + 4 + 256 + 121*sps
 * samples (up to 7 more: the next buffer starts on a multiple of 8 samples).  One call pushes the next chunk of ANY SUBSET of
 * the streams through one k_batch launch: a small kernel in front of it assembles every item's buffer [stream carry | new chunk]
 * (the host entry point uploads the chunks straight into place; the device entry point's chunks are copied by that kernel),
 * one behind the pack step keeps each buffer's last samples for the next call.
 * With F = 256 + 121*sps, the call that appends samples [pos, pos + n) owns the pulse rises of [pos - F, pos + n - F) (the
 * first call owns from the stream's start): output is delayed by the look-ahead F, as in blocks.framer(improved=True).  An
 * item flagged ADSB_STREAM_END owns up to the end of the stream and applies the end-of-call rules (framer.py:102-108,
 * demod.py:82); after it the stream is fresh again (pos 0, nothing carried, the same base).
 * CONTRACT: for a stream whose threshold is constant and in which no owned pulse is still high at the end of its call's
 * buffer, the concatenation of its records over all calls, the END item included, is byte-identical to adsb_process_format
 * over the concatenation of its chunks -- same records, order and flags, for ANY chunking (n == 0 included).  A threshold
 * that changes between calls applies to the rises the call owns.
 * DEVIATION: the carry is bounded.  A pulse that is still high at the end of its call's buffer, and a burst whose last bit
 * lies at or beyond it, is left out (as ADSB_SHARD_DROP_OVERLONG does) and counted in the stream's n_overlong.
 * Output as adsb_process_batch: out[item_first[i] .. item_first[i+1]) belong to item i.  -ENOSPC with *n_out = the number
 * needed when cap is too small: NO stream has moved, the same call can be repeated with more room.  Items whose buffer exceeds
 * ADSB_BATCH_ITEM_MAX samples or whose lists overflow run through the ordinary pass with the same plan and carried state
 * (*n_fallback).  -EINVAL: a stream twice in one call, an unknown stream, a format other than the one the stream started with,
 * n < 0, device data not aligned to a sample, reserved != 0, unknown flags, no open streams, ADSB_FLAG_AIRCRAFT_TABLE / _DECODE
 * / _CONFIDENCE contexts; -EBUSY while tickets are pending.  ADSB_FLAG_LONG_AWARE_GATE and ADSB_FLAG_FEC_CONSERVATIVE apply as
 * in the batch.  adsb_reset makes every stream fresh.  adsb_last_result and the framer state are left alone.  No reference
 * counterpart. */
#define ADSB_STREAM_END 1u /* adsb_stream_item.flags: the stream's last item */
typedef struct adsb_stream_item {
  const void* data;   /* the next n samples: host memory (adsb_process_stream_batch) or device-readable, aligned to a sample (.._device) */
  int64_t n;          /* samples; 0 is legal, with and without ADSB_STREAM_END */
  int32_t stream;     /* 0 .. n_streams - 1; at most once per call */
  uint32_t flags;     /* ADSB_STREAM_END or 0 */
  float threshold;    /* the framer threshold for the rises this call owns */
  uint32_t reserved;  /* must be 0 */
} adsb_stream_item;   /* 32 bytes */
int adsb_streams_open(adsb_ctx* ctx, int32_t n_streams);  /* n fresh streams with base 0; -EINVAL while streams are open */
int adsb_streams_close(adsb_ctx* ctx);                    /* releases the carry store and the call buffers */
int adsb_stream_set_base(adsb_ctx* ctx, int32_t stream, int64_t abs_offset); /* fresh streams only */
int adsb_stream_state(adsb_ctx* ctx, int32_t stream, int64_t* pos, int64_t* eob, int64_t* n_overlong); /* any pointer may be NULL */
int adsb_stream_reset(adsb_ctx* ctx, int32_t stream);     /* fresh again: pos 0, nothing carried, n_overlong 0; the base stays */
int adsb_process_stream_batch(adsb_ctx* ctx, int format, const adsb_stream_item* items, int32_t n_items, adsb_burst* out,
                              int32_t cap, int32_t* item_first, int32_t* n_out, int32_t* n_fallback);
int adsb_process_stream_batch_device(adsb_ctx* ctx, int format, const adsb_stream_item* items, int32_t n_items, adsb_burst* out,
                                     int32_t cap, int32_t* item_first, int32_t* n_out, int32_t* n_fallback);
/* STREAM DECODERS (ADSB_FLAG_STREAM_DECODE).  adsb_streams_open also gives every stream a decoder of its own -- what
 * ADSB_FLAG_AIRCRAFT_TABLE | ADSB_FLAG_DECODE is for one receiver -- and adsb_streams_close releases them.  Their state is ONE
 * sparse store on the device, keyed by (stream, address): open addressing over a power-of-two number of 104-byte slots (the
 * key, the address's first announcement, the 88-byte plane), at most half of them taken, at most 2^27.  Only a reply that
 * announces its address takes a slot -- every reply that reaches update_plane does --; address/parity replies with unheard
 * addresses (noise) take none.  Before a call's decode step the store holds room for one slot per record of the call, or it
 * is rehashed: the live slots move to a new store, the slots of reset streams are dropped, the old store is freed.  The new
 * store has the same size unless the LIVE slots plus the call's records would take more than half of it; then it is doubled
 * until they do not, which is a growth (counted: adsb_stream_decoder_stats).  A rehash changes no row.  The store never
 * shrinks (adsb_stream_planes_expire frees slots, not memory).  Nothing runs out in a long-lived fleet: the call numbers that order announcements start over at a rehash
 * before 2^32 calls are reached, with every announcement made so far kept as "earlier".
 * CONTRACT: for every stream s -- any chunking, any subset of streams per call, n == 0 and END items included -- the
 * concatenation of its records over all calls is byte-identical to what an ADSB_FLAG_AIRCRAFT_TABLE | ADSB_FLAG_DECODE context
 * with the same ADSB_FLAG_FEC_CONSERVATIVE / _LONG_AWARE_GATE flags, format scale and adsb_set_decoder(msg_filter, start_s)
 * writes for ONE adsb_process_format call over the concatenation of s's chunks (ADSB_BURST_AP_KNOWN / _AP_FEC included), and
 * the concatenation of its rows is byte-identical to that context's adsb_last_decoded (records left out as n_overlong are
 * left out of both).  Streams never see each other's aircraft, whatever addresses they share.  Publication order inside a
 * stream is call order, within a call the order of its records.  A record's PDU timestamp is
 * start_s + (double)offset / fs with the record's offset (the stream's base included); the decoder's clock is
 * (long long)timestamp as for ADSB_FLAG_DECODE.
 * The decode step runs on the call's final record list (the records of items that took the ordinary pass included), and only
 * once the call is known to be delivered: a call that returns -ENOSPC or any other error has changed no decoder state.
 * adsb_stream_reset also makes that stream's decoder fresh (a new generation in the store's key: O(1) on the host; every
 * 2^20 - 2 resets of one stream the store is rehashed); adsb_reset does so for every stream; an ADSB_STREAM_END item does
 * NOT: the aircraft are still there when the receiver reconnects.  At most 2^20 streams. */
/* SHARED DECODER (ADSB_FLAG_STREAM_DECODE | ADSB_FLAG_STREAM_DECODE_SHARED): the streams keep their own framing state and
 * feed ONE decoder.  For one delivered adsb_process_stream_batch[_device] call with final record list out[0 .. n), let
 *   ts[t] = start[stream of t] + (double)offset[t] / fs        (adsb_stream_set_start; the offset with the stream's base).
 * PUBLICATION ORDER: within the call ascending (ts[t], t) -- time first, ties in the list order of the call, which is the
 * order of the items as the caller passed them and then the position, NOT the stream index.  Records without
 * ADSB_BURST_DEMOD take part in the order and publish nothing.  Calls publish in call order: a later call may carry earlier
 * timestamps, and the decoder then sees time go backwards, as adsb_decode_pdus allows.
 * EQUIVALENCE: the records' ADSB_BURST_AP_KNOWN / _AP_FEC flags and the rows of adsb_stream_last_decoded are byte-identical
 * to what ONE reference-equivalent decoder (msg_filter of adsb_streams_set_decoder; error_corr "Conservative" iff
 * ADSB_FLAG_FEC_CONSERVATIVE) gives when fed exactly that PDU sequence with those timestamps.  Row t still belongs to
 * out[t]; item_first and the order of the records in out are those of a context without the flag.
 * As for STREAM DECODERS: a call that returns -ENOSPC or any other error has changed no decoder state; items that took the
 * ordinary pass are decoded with the rest; n == 0 and ADSB_STREAM_END items are legal; growth and rehash change no row.
 * STATE: the decoder lives in the store under stream index 0 and that index's generation, and every plane entry point
 * reports it as stream 0's -- adsb_stream_planes[_seen], adsb_stream_planes_expire, adsb_stream_planes_merged,
 * adsb_stream_decoder_stats --; all other streams hold nothing (adsb_stream_planes with streams == NULL: first[] =
 * 0, n, n, ...).  adsb_stream_reset(s) resets stream s's framing state only; adsb_reset and adsb_streams_decoder_reset make
 * the decoder fresh; an ADSB_STREAM_END item leaves it alone.
 * The same reply heard by several receivers is published once per hearing, as in the reference's fan-in: num_msgs counts
 * every hearing -- unless the context has ADSB_FLAG_STREAM_DEDUP: see DE-DUPLICATION below.
 * ADSB_ABI_VERSION is unchanged: a flag and entry points only. */
/* order[r]: the list position of the r-th record in the publication order of the last DELIVERED stream-batch call (*n = that
 * call's *n_out; *order NULL when 0).  Pinned memory of the context, valid until the next DELIVERED stream-batch call: a
 * call that fails leaves the pointer and what it points to alone.  -EINVAL on a
 * context without ADSB_FLAG_STREAM_DECODE_SHARED or without open streams. */
int adsb_stream_last_order(adsb_ctx* ctx, const int32_t** order, int32_t* n);
/* A fresh shared decoder in O(1): a new generation of the store's key, as adsb_stream_reset gives one stream's decoder on a
 * context without the shared flag.  The streams' framing state stays.  -EINVAL without ADSB_FLAG_STREAM_DECODE_SHARED or
 * without open streams. */
int adsb_streams_decoder_reset(adsb_ctx* ctx);
int adsb_streams_set_decoder(adsb_ctx* ctx, int32_t msg_filter);   /* ADSB_DEC_*, for all streams; default ADSB_DEC_ALL_MESSAGES */
/* DE-DUPLICATION (ADSB_FLAG_STREAM_DEDUP on a shared decoder): a reply that k receivers hear is published once, not k times.
 * THE RULE.  A record TAKES PART if it has ADSB_BURST_DEMOD.  Its PAYLOAD is its bits[] as the decode step receives them
 * (with ADSB_BURST_FEC_FIXED: the repaired reply): the first 112 bits if ADSB_BURST_LONG is set, otherwise the first 56 bits
 * only -- a short reply's bytes 7..13 are sliced noise and differ between receivers.  Two payloads are equal when their
 * lengths and those bits are equal.  With ts[t] = start[stream] + (double)offset / fs as above, record r is a DUPLICATE iff
 * there is a record q that takes part, is EARLIER IN PUBLICATION ORDER (an earlier delivered call, or the same call and
 * earlier in ascending (ts, list position)), is still held by the carry (below), comes from a DIFFERENT STREAM, has an equal
 * payload, and satisfies fabs(ts[r] - ts[q]) <= window, evaluated in double with exactly that expression.  q may itself be
 * a duplicate: the rule depends on the inputs only, never on earlier verdicts, so one thread per record evaluates it.
 * CONSEQUENCES.  Of a set of hearings from distinct streams that lie pairwise within window, exactly the first in
 * publication order is published, for any chunking within the horizon.  The same payload twice on the SAME stream is two
 * transmissions: both are published.  A context with one stream never marks anything.
 * A DUPLICATE publishes nothing: no slot, no plane update, no num_msgs, no last_seen.  Its delivered record is that of a
 * context without a decoder (ADSB_BURST_DEMOD kept, never ADSB_BURST_AP_KNOWN / _AP_FEC); its row is the row of a record
 * without ADSB_BURST_DEMOD with port = ADSB_DEC_DUPLICATE; it keeps its place in order[].
 * EQUIVALENCE, extending the shared decoder's: the flags and rows of all other records are byte-identical to ONE reference
 * decoder fed the publication sequence with the duplicates left out.
 * THE CARRY.  The hearings of one reply fall into different calls, so the context keeps a time-sorted carry on the device:
 * every record of earlier delivered calls (duplicates included) with ts >= hi - horizon, where hi is the largest timestamp
 * of any record delivered since the decoder was last fresh; the cut is applied at the end of each delivered call, with that
 * double expression.  A record of a later call is compared against carry entries on both sides in time (hence the fabs).
 * A hearing that arrives after hi has moved more than horizon past it is published again: that is the bound.
 * adsb_streams_decoder_reset and adsb_reset clear the carry and hi; adsb_stream_reset (framing only), ADSB_STREAM_END items,
 * adsb_stream_planes_expire and any call that fails (-ENOSPC, any error) leave both alone.
 * COST: O(n x records within window) comparisons per call, plus O((n + carried) log) for the merge: the whole carry -- every
 * record of the last `horizon` seconds -- is read and rewritten by every delivered call, so a long horizon on a dense fleet is
 * what a call pays for (DESIGN.md 3h measures it).
 * adsb_streams_set_dedup: window_s and horizon_s in seconds.  Defaults 0.002 and 1.0: 400 km of differential path are 1.3 ms,
 * the rest is clock error between receivers; the horizon covers the lag between the receivers' deliveries.  window = 0 is
 * legal: bit-equal timestamps only.  -EINVAL for NaN, negative values or horizon < window; without the flag or without open
 * streams; and once a call with records has been delivered since the decoder was last fresh. */
int adsb_streams_set_dedup(adsb_ctx* ctx, double window_s, double horizon_s);
/* Beside adsb_stream_last_order, with its lifetime rules: dup[t] of the last DELIVERED call.  -1: position t is not a
 * duplicate; -2: some matching q lies in an earlier call; otherwise the list position of the earliest-published matching q
 * of this call. */
int adsb_stream_last_duplicates(adsb_ctx* ctx, const int32_t** dup, int32_t* n);
/* duplicates: since the decoder was last fresh; carried: entries the carry holds now; hi: as above (0 while nothing has been
 * delivered).  Any pointer may be NULL.  -EINVAL without the flag or without open streams. */
int adsb_stream_dedup_stats(adsb_ctx* ctx, int64_t* duplicates, int64_t* carried, double* hi);
/* MULTILATERATION (ADSB_FLAG_STREAM_DEDUP contexts; entry points only: nothing runs unless a caller asks, and
 * ADSB_ABI_VERSION is unchanged).  The carry of DE-DUPLICATION holds, for `horizon` seconds, every hearing of every reply with
 * its arrival time and its stream.  Four hearings and the receivers' positions give the transmitter's position, whether or
 * not the reply announces one: adsb_stream_mlat groups the carry's hearings and solves each group on the device.  It changes
 * no state: the carry, hi, the decoder, adsb_stream_last_* and the framer state are untouched, and two calls with nothing
 * between them are byte-identical.  No reference counterpart (the reference is one receiver).
 * THE GROUP RULE depends on the carry only, in carry order: ascending ts, ties as the carry keeps them (the merge is stable,
 * the carry first, a call's records in publication order).  An entry TAKES PART as in DE-DUPLICATION (its record had
 * ADSB_BURST_DEMOD); the others are skipped everywhere below.  Two payloads are equal as in DE-DUPLICATION: the same length
 * and the same bits of that length.  An entry is a HEAD iff no entry q in front of it in carry order, from ANY stream, has
 * an equal payload and ts_head - ts_q <= window.  The head's GROUP is the head plus the entries m behind it in carry order
 * with an equal payload and ts_m - ts_head <= window; both tests in double with exactly those expressions, window being
 * the context's de-duplication window.  The head and the first 63 other entries of the group, in carry order, are its
 * CANDIDATES.  A candidate is USED iff no candidate in front of it has its stream and its stream has a position
 * (adsb_stream_set_ecef).  n_heard counts the whole group, n_rx the used hearings.  An entry that is neither a head nor in a
 * head's group belongs to nothing: of a chain a - b - c with c beyond the window from a, b is in a's group and c, which b
 * precedes within the window, is no head and in no group.  Groups are disjoint.
 * THE SOLVER.  All arithmetic in double, no contraction.  With R_i the receiver of used hearing i (carry order) and
 * C = ADSB_MLAT_C: d_i = C * (ts_i - ts_head), the difference first.  Unknowns: the position p and b = C * (ts_head - t_tx).
 * Residual r_i = |p - R_i| - d_i - b.  Start: c = the mean of the R_i; p0 = c + 10000 * c / |c| (10 km further from the
 * Earth's centre); b0 = |p0 - R_0|, R_0 being the first used hearing's receiver (the head's, when the head is used).
 * Gauss-Newton: row i of J is ((p - R_i) / |p - R_i|, -1); solve (J^T J) delta = -J^T r by Cholesky, the pivots in the
 * order x, y, z, b; a pivot that is not finite and positive ends the solve with ADSB_MLAT_SINGULAR, the iterate as it was.
 * Otherwise (p, b) += delta, iters += 1, and |delta_p| < 0.001 m ends it with ADSB_MLAT_OK; 32 iterations without that
 * give ADSB_MLAT_NO_CONVERGE.  rms_m = sqrt(sum r_i^2 / n_rx) at the last iterate, t_tx = ts_head - b / C.  The sums over the
 * hearings are taken across a wavefront; their order is the implementation's, so positions agree with another evaluation of
 * this rule to the solve's own sensitivity (tests/test_mlat.py measures it), everything else exactly.
 * A fix says where the rule's arithmetic ended, not that the aircraft is there: judge it by status, rms_m, n_rx and the
 * receivers' geometry.  Four receivers in a plane leave the height weak.
 * PRECISION.  An arrival time is the carry's ts = start + (double)offset / fs.  It carries the sample period (150 m at
 * 2 Msps, 15 m at 20 Msps) and the double's ulp at the magnitude of start: 238 ns, about 71 m, for Unix-epoch starts.  MLAT
 * users should pass starts relative to a session epoch: below 2^23 s the ulp is under 1 ns (0.3 m).  The decoder's
 * last_seen clock works the same either way.  adsb_stream_mlat_stats reports C * ulp(hi), so a caller can see the limit.
 * Sub-sample arrival times, clock offsets between receivers and altitudes other than the reply's own barometric one (DF 18,
 * GNSS height) are not provided.  (Fixes are fused per aircraft by MLAT TRACKS, below.)
 * THE DAMPED RULE (adsb_stream_mlat_rule with ADSB_MLAT_SOLVER_LM; THE SOLVER above is ADSB_MLAT_SOLVER_GN and stays as it is).
 * Grouping, candidates, USED, d_i, b, the residuals r_i, the rows of J and the arithmetic (double, no contraction) are
 * unchanged.  c = the mean of the R_i, u = c / |c|, up(p) = (p - c) . u.
 * A DAMPED RUN from a start p: b = |p - R_0|, lambda = 1e-3, S = sum r^2 over all rows.  At most 64 TRIALS.  A trial forms
 * A = J^T J and g = J^T r at the iterate, multiplies A's diagonal by (1 + lambda), factors it by Cholesky in the order x, y,
 * z, b -- a pivot that is not finite and positive ends the run with ADSB_MLAT_SINGULAR, the iterate as it was -- solves
 * A delta = -g and sets tries += 1.  THE UNTESTED LAST STEP: if |delta_p| < 0.001 m and lambda <= 1e-3 the step is taken as it
 * is -- the iterate moves, iters += 1 -- and the run ends with ADSB_MLAT_OK: at that damping the step is THE SOLVER's to a
 * thousandth, and THE SOLVER stops there too; S' against S would be decided by rounding alone there (S sits at its floor), and
 * a rule that asked would reject such steps at random and count them.  Otherwise the trial evaluates S' = sum r^2 at
 * (p + delta_p, b + delta_b).  If S' is finite and S' <= S the step is taken: the iterate moves, S = S', iters += 1,
 * lambda = max(lambda / 10, 1e-12), and |delta_p| < 0.001 m ends the run with ADSB_MLAT_OK.  Otherwise the iterate stays,
 * lambda *= 10, and lambda > 1e12 ends the run with ADSB_MLAT_NO_CONVERGE.
 * 64 trials without an end give ADSB_MLAT_NO_CONVERGE.  rms_m = sqrt(sum r_i^2 / n_rx) over the timing rows only, at the
 * last iterate; t_tx as above.  iters counts the steps taken.
 * THE RESTART (ADSB_MLAT_RESTART; unaided groups only).  The first run starts at c + 10000 u, as THE SOLVER does.  If it does
 * not end ADSB_MLAT_OK a second run starts at c + 30000 u; if it ends ADSB_MLAT_OK with up(p) < 0 -- below the receivers: the
 * mirror image -- a second run starts at the mirror p - (2 up(p)) u.  The second run's result replaces the first's (position,
 * b, status, iters, lambda, up_m) iff it ends ADSB_MLAT_OK with up >= 0.  tries counts the trials of every run made.
 * THE ALTITUDE ROW (ADSB_MLAT_ALTITUDE).  The head's payload gives alt_ft by the decoder's own rule: DF 0 / 4 / 16 / 20, bits
 * 19..31 (13 bits: none if the field is 0, M (0x40) is set or Q (0x10) is clear; else the other 11 bits * 25 - 1000); DF 17
 * with type code 9..18, bits 40..51 (12 bits: none if Q (0x10) is clear; else the other 11 bits * 25 - 1000); any other reply:
 * none.  A group with an altitude is AIDED: every run has one more row, r_a = w * (h(p) - 0.3048 * alt_ft) with the Jacobian
 * row (w * n(p), 0), w = alt_weight: metres of range per metre of height -- pressure altitude is not height above the
 * ellipsoid, so the caller says how far to trust it.  The row adds w^2 n n^T to the position block of A (before the damping),
 * w n r_a to g and r_a^2 to S and S'; A's b row and column are unchanged.  h and n come from ONE Bowring step on WGS-84 (a,
 * f; e2 = f (2 - f), bp = a (1 - f), ep2 = e2 / (1 - e2)), written with sqrt and / only: q = sqrt(x^2 + y^2);
 * t = (z a) / (q bp); cb = 1 / sqrt(1 + t^2), sb = t cb; T = (z + ep2 bp sb^3) / (q - e2 a cb^3); cp = 1 / sqrt(1 + T^2),
 * sp = T cp; h = q cp + z sp - a sqrt(1 - e2 sp^2); n = (cp x / q, cp y / q, sp).  (On the polar axis q = 0, nothing is finite
 * and the run ends ADSB_MLAT_SINGULAR.)  An aided group takes no restart.  A group of three used hearings is solved only when
 * it is aided; otherwise it is not returned -- it is no row, and it counts neither in *n_fixes nor in *n_members.  Without
 * ADSB_MLAT_ALTITUDE no payload is read for an altitude and alt_ft is -1.
 * adsb_stream_mlat_rule is adsb_stream_mlat with the rule stated by the caller: the same range, rows, member lists, ordering
 * and errors, and it changes no state either.  rule->solver ADSB_MLAT_SOLVER_GN with flags 0 and min_rx >= 4 returns byte for
 * byte what adsb_stream_mlat(..., min_rx, ...) returns (aux rows, if asked for: alt_ft -1, everything else 0).  -EINVAL also
 * for: rule NULL; a solver other than _GN / _LM; unknown flag bits; any flag with _GN; reserved != 0; min_rx < 4, or < 3
 * with ADSB_MLAT_ALTITUDE; with ADSB_MLAT_ALTITUDE an alt_weight that is not finite and > 0.  aux (may be NULL): one row
 * beside each fix -- up_m: up(p) of the returned position (negative: below the receivers); lambda: the kept run's last
 * damping; alt_ft; tries; flags: ADSB_MLAT_AUX_AIDED, ADSB_MLAT_AUX_RESTARTED (a second run was made), ADSB_MLAT_AUX_SECOND_KEPT.
 * adsb_stream_set_ecef: the antenna of `stream` in WGS-84 ECEF metres.  Allowed at any time while streams are open; it is
 * not decoder state: adsb_stream_reset, adsb_streams_decoder_reset and adsb_reset keep it, adsb_streams_close forgets it.
 * -EINVAL for non-finite values, a bad stream, or a context without ADSB_FLAG_STREAM_DEDUP.  A stream without a position
 * never contributes a hearing.
 * adsb_stream_mlat solves every group whose head has t_lo <= ts < t_hi (infinities open a side; the members may lie beyond
 * t_hi) and n_rx >= min_rx; rows in carry order of the heads; the members of row j are member_stream / member_ts[first ..
 * first + n_rx), in carry order.  min_rx < 4, NaN bounds, a context without the flag or without open streams: -EINVAL;
 * -EBUSY while submitted tickets are pending.  cap or member_cap too small: -ENOSPC with the needed counts in *n_fixes and
 * *n_members and nothing written (fixes == NULL with cap == 0 and member_cap == 0 is a count query).  An empty carry or
 * range: 0 rows.  The call is ordered behind the last delivered stream-batch call. */
#define ADSB_MLAT_C 299702547.0 /* m/s: the speed of light / 1.0003 */
#define ADSB_MLAT_OK 0
#define ADSB_MLAT_NO_CONVERGE 1
#define ADSB_MLAT_SINGULAR 2
typedef struct adsb_mlat_fix { /* 88 bytes */
  double ts;                   /* the head's timestamp */
  double x, y, z;              /* the last iterate: WGS-84 ECEF metres (adsb_ecef_to_geodetic) */
  double t_tx;                 /* the estimated transmit time */
  double rms_m;                /* the residual at the last iterate */
  uint8_t bits[14];            /* the head's payload, masked to its length */
  uint16_t flags;              /* ADSB_BURST_LONG or 0 */
  int32_t icao;                /* DF 11/17/18: bytes 1..3; DF 0/4/5/16/20/21: the remainder of the whole reply (the address under
                                  address/parity: adsb_mode_s_syndrome); any other DF: -1 */
  int32_t n_rx, n_heard;
  int32_t status;              /* ADSB_MLAT_* */
  int32_t iters;
  int32_t first;
} adsb_mlat_fix;
int adsb_stream_set_ecef(adsb_ctx* ctx, int32_t stream, double x, double y, double z);
int adsb_stream_mlat(adsb_ctx* ctx, double t_lo, double t_hi, int32_t min_rx, adsb_mlat_fix* fixes, int32_t cap, int32_t* n_fixes,
                     int32_t* member_stream, double* member_ts, int32_t member_cap, int32_t* n_members);
#define ADSB_MLAT_SOLVER_GN 0
#define ADSB_MLAT_SOLVER_LM 1
#define ADSB_MLAT_RESTART 1
#define ADSB_MLAT_ALTITUDE 2
#define ADSB_MLAT_AUX_AIDED 1u
#define ADSB_MLAT_AUX_RESTARTED 2u
#define ADSB_MLAT_AUX_SECOND_KEPT 4u
typedef struct adsb_mlat_rule { /* 24 bytes */
  int32_t solver;              /* ADSB_MLAT_SOLVER_* */
  int32_t flags;               /* ADSB_MLAT_RESTART | ADSB_MLAT_ALTITUDE: ADSB_MLAT_SOLVER_LM only */
  int32_t min_rx;              /* >= 4; >= 3 with ADSB_MLAT_ALTITUDE */
  int32_t reserved;            /* 0 */
  double alt_weight;           /* finite and > 0 with ADSB_MLAT_ALTITUDE; otherwise not read */
} adsb_mlat_rule;
typedef struct adsb_mlat_aux { /* 32 bytes */
  double up_m, lambda;
  int32_t alt_ft;              /* -1: none */
  int32_t tries;
  uint32_t flags;              /* ADSB_MLAT_AUX_* */
  int32_t reserved;
} adsb_mlat_aux;
int adsb_stream_mlat_rule(adsb_ctx* ctx, double t_lo, double t_hi, const adsb_mlat_rule* rule, adsb_mlat_fix* fixes, adsb_mlat_aux* aux,
                          int32_t cap, int32_t* n_fixes, int32_t* member_stream, double* member_ts, int32_t member_cap, int32_t* n_members);
/* positioned: streams with a position; ts_ulp_m: ADSB_MLAT_C * ulp(hi), what the double's spacing at the carry's latest
 * timestamp is worth in metres.  Either pointer may be NULL.  -EINVAL without the flag or without open streams. */
int adsb_stream_mlat_stats(adsb_ctx* ctx, int32_t* positioned, double* ts_ulp_m);
/* MLAT TRACKS (ADSB_FLAG_STREAM_DEDUP contexts; entry points only: nothing runs and nothing is allocated unless a caller asks).
 * A store of TRACKS on the device, one per 24-bit address, that outlives the carry: a position p and a velocity v in ECEF
 * metres and metres per second, the time last_ts of the last fix it took, and counters.  Fixes enter it by the sequential,
 * outlier-gated rule below; it is read back in ascending icao, as the plane snapshots are.  Time is the fix's ts (the head's
 * timestamp) throughout.
 * THE RULE.  One adsb_stream_mlat_track call runs the caller's adsb_mlat_rule over the heads with t_lo <= ts < t_hi exactly
 * as adsb_stream_mlat_rule would -- the same rows in the same order; they stay on the device -- and takes the ELIGIBLE fixes
 * (icao >= 0) per address in ascending row order: carry order, which is ascending ts with ties in row order.  Each fix f in
 * turn meets its address's track T.  All arithmetic is in double with no contraction; |a| = sqrt(a.x*a.x + a.y*a.y + a.z*a.z),
 * summed in that order.
 * 1. USABLE iff status == ADSB_MLAT_OK, x, y, z and rms_m are finite, rms_m <= max_rms_m and aux.up_m >= min_up_m (under
 *    ADSB_MLAT_SOLVER_GN up_m is 0, so min_up_m <= 0 admits those fixes).  A fix that is not usable counts in unusable only.
 * 2. STALE: if T exists and f.ts <= T.last_ts the fix counts in stale only.  So a fix a track has taken is never taken
 *    twice: a second call over the same range finds every such fix stale and changes no byte of the store.  (A REJECTED fix
 *    does not move last_ts and is not remembered: a later call whose range covers it gates it again and counts it again.
 *    Where outliers matter, let the ranges of successive calls adjoin rather than overlap.)
 * 3. START: if T does not exist, or f.ts - T.last_ts > max_gap_s: p = f, v = 0, first_ts = last_ts = f.ts, n_fixes = 1,
 *    misses = 0, rms_m and n_rx the fix's; n_rejected and flags are 0 on a new track and kept on a gap restart, which also sets
 *    ADSB_TRACK_GAP.
 * 4. GATE: otherwise dt = f.ts - last_ts, pp = p + v*dt, d = f - pp.  REJECTED iff |d| > gate_m + max_speed_mps * dt: n_rejected
 *    and misses grow by 1; if misses has reached restart_after the track restarts at this fix as in START with
 *    ADSB_TRACK_RESTARTED set (how a track begun on a mirror root or an outlier recovers); otherwise nothing else of T changes.
 * 5. STEP: otherwise p = pp + alpha*d, v = v + (beta/dt)*d, last_ts = f.ts, n_fixes += 1, misses = 0, rms_m and n_rx the fix's.
 * LIMITS.  The gains are fixed: this is an alpha-beta filter, not a Kalman filter; there is no per-fix covariance, and a fix's
 * weak height enters as it is.  The velocity is only as good as the fixes' scatter over the time they span.  A corrupted
 * address/parity reply gives a garbage icao and so a one-fix track: readers filter by min_fixes, and expiry removes such
 * tracks.  The Python layer's default gains were tried against one simulated aircraft (DESIGN.md 3j says how); that is one
 * simulation, not a measurement of real traffic.
 * adsb_stream_mlat_track changes the track store and nothing else: the carry, hi, the decoder, adsb_stream_last_* and the framer
 * state stay as they were.  stats (may be NULL): fixes = the rows adsb_stream_mlat_rule would return; eligible; unusable; stale;
 * rejected; taken = the STEP fixes; started = the START fixes, restarts of both kinds included (a fix that is rejected and
 * restarts its track counts in rejected and in started); tracks = the store's rows after the call.  It refuses what
 * adsb_stream_mlat_rule refuses, with the same codes; -EINVAL also for: track_rule NULL; alpha or beta not finite or outside
 * (0, 1]; gate_m, max_speed_mps or max_gap_s negative or not finite; max_rms_m or min_up_m NaN; restart_after < 1;
 * reserved != 0.  A refused call changes no track.  The store is allocated by the first call that needs it and grows on the
 * host's decision before the launch that needs the room.
 * adsb_stream_mlat_tracks: the tracks with n_fixes >= min_fixes and last_ts >= cutoff (-inf: all; NaN: -EINVAL) into
 * rows[0 .. *n), ascending icao.  cap too small: -ENOSPC with the count in *n and nothing written (rows == NULL with
 * cap == 0 is a count query).  It changes nothing.
 * adsb_stream_mlat_tracks_expire removes the tracks with last_ts < cutoff (their number in *n_removed, may be NULL); a later
 * fix of such an address starts a new track.  adsb_stream_mlat_tracks_reset forgets every track.
 * The store is not decoder state: adsb_stream_reset, adsb_streams_decoder_reset and adsb_reset keep it;
 * adsb_stream_mlat_tracks_reset and adsb_streams_close forget it.  All four calls: -EBUSY while submitted tickets are
 * pending; -EINVAL without ADSB_FLAG_STREAM_DEDUP or without open streams. */
#define ADSB_TRACK_GAP 1u
#define ADSB_TRACK_RESTARTED 2u
typedef struct adsb_mlat_track_rule { /* 64 bytes */
  double alpha, beta;          /* the gains of position and velocity: (0, 1] */
  double gate_m, max_speed_mps; /* the gate |d| <= gate_m + max_speed_mps * dt: >= 0 */
  double max_gap_s;            /* a longer silence restarts the track: >= 0 */
  double max_rms_m, min_up_m;  /* what makes a fix usable */
  int32_t restart_after;       /* >= 1: rejected fixes in a row before the track restarts */
  int32_t reserved;            /* 0 */
} adsb_mlat_track_rule;
typedef struct adsb_mlat_track { /* 96 bytes */
  int32_t icao;
  uint32_t flags;              /* ADSB_TRACK_* */
  int32_t n_fixes;             /* taken since the last start, that one included */
  int32_t n_rejected;
  double first_ts, last_ts;    /* of the last start; of the last fix taken */
  double x, y, z;              /* WGS-84 ECEF metres at last_ts */
  double vx, vy, vz;           /* metres per second */
  double rms_m;                /* of the last fix taken */
  int32_t n_rx;                /* of the last fix taken */
  int32_t misses;              /* rejected fixes since the last one taken */
} adsb_mlat_track;
typedef struct adsb_mlat_track_stats { /* 64 bytes */
  int64_t fixes, eligible, unusable, stale, rejected, taken, started, tracks;
} adsb_mlat_track_stats;
int adsb_stream_mlat_track(adsb_ctx* ctx, double t_lo, double t_hi, const adsb_mlat_rule* rule, const adsb_mlat_track_rule* track_rule,
                           adsb_mlat_track_stats* stats);
int adsb_stream_mlat_tracks(adsb_ctx* ctx, int32_t min_fixes, double cutoff, adsb_mlat_track* rows, int32_t cap, int32_t* n);
int adsb_stream_mlat_tracks_expire(adsb_ctx* ctx, double cutoff, int64_t* n_removed);
int adsb_stream_mlat_tracks_reset(adsb_ctx* ctx);
/* WGS-84 (a = 6378137 m, f = 1 / 298.257223563), degrees and metres, plain host arithmetic in double.  The inverse is
 * Bowring's start followed by three fixed-point rounds on the latitude; at the poles longitude is 0.  No context. */
void adsb_geodetic_to_ecef(double lat_deg, double lon_deg, double alt_m, double* x, double* y, double* z);
void adsb_ecef_to_geodetic(double x, double y, double z, double* lat_deg, double* lon_deg, double* alt_m);
int adsb_stream_set_start(adsb_ctx* ctx, int32_t stream, double start_timestamp);   /* fresh streams only; default 0 */
/* Row t belongs to out[t] of the last DELIVERED adsb_process_stream_batch[_device] call (*n = that call's *n_out; *rows NULL
 * when 0).  Pinned memory of the context, valid until the next stream-batch call. */
int adsb_stream_last_decoded(adsb_ctx* ctx, const adsb_decoded** rows, int32_t* n);
/* The store's capacity in slots: rounded up to a power of two that is at least 256 (65536 after adsb_streams_open).  Allowed
 * while streams are open and no slot is live (-EINVAL otherwise, and above 2^27). */
int adsb_stream_decoder_reserve(adsb_ctx* ctx, int64_t slots);
/* planes: plane_dict entries of all streams' decoders together (exact: a reset stream's are gone at once); capacity: slots;
 * grows: growths since adsb_streams_open.  Any pointer may be NULL.  -EINVAL without the flag or without open streams. */
int adsb_stream_decoder_stats(adsb_ctx* ctx, int64_t* planes, int64_t* capacity, int64_t* grows);
/* PLANE SNAPSHOTS: the decoders' plane_dict (decoder.py:413-449) read back from the device, for one decoder (adsb_planes:
 * ADSB_FLAG_DECODE contexts, -EINVAL on others) and for a fleet (adsb_stream_planes: ADSB_FLAG_STREAM_DECODE contexts with open
 * streams, -EINVAL otherwise).  Entry points only: nothing runs unless a caller asks, and ADSB_ABI_VERSION is unchanged.
 * A snapshot row is an adsb_decoded row: port = ADSB_DEC_NONE, df = 0, bits and every pad byte zero, icao = the address;
 * present (always with ADSB_DEC_HAS_PLANE), callsign, altitude, velocity_we, velocity_sn, vertical_rate, latitude, longitude
 * and num_msgs hold exactly what the row of a record that touches the plane would show at this moment.  The CPR frames
 * (plane_dict's "cpr") and last_seen are NOT part of a snapshot row (print_planes, decoder.py:452-509, prints neither);
 * an ADSB_FLAG_PLANE_AGES context returns last_seen beside the rows: adsb_planes_seen, adsb_stream_planes_seen.
 * adsb_planes: every address whose plane exists in the context's current epoch, in ascending address order; nothing after
 * adsb_reset; an address that was announced but has no plane is not returned.
 * adsb_stream_planes: streams == NULL selects all n_streams streams (n_sel is ignored and counts as n_streams); otherwise
 * streams[0 .. n_sel) are stream indices in strictly ascending order (-EINVAL when out of range or not ascending).  Rows are
 * ordered by (stream, address).  first may be NULL; else first[i] .. first[i + 1] are the rows of the i-th selected stream
 * (n_sel + 1 entries, first[n_sel] == *n_out: item_first's convention).  A stream's planes are those of its current
 * generation: adsb_stream_reset removes them at once (its slots stay in the store until the next rehash), an ADSB_STREAM_END
 * item does not, and streams never show each other's aircraft.
 * Both: cap smaller than the number of planes is -ENOSPC with *n_out = the number needed and nothing written (rows == NULL
 * with cap == 0 is a count query); -EBUSY while submitted tickets are pending.  A snapshot is taken behind the last queued
 * table or decode step (it waits on their event chain), so it reflects every delivered call and every adsb_decode_pdus call
 * that returned before it, and nothing else.  It changes no state: rows decoded after it are byte-identical to rows
 * decoded without it, two snapshots with nothing between them are byte-identical, and adsb_last_result, adsb_last_decoded,
 * adsb_stream_last_decoded and the framer state are untouched.  No reference counterpart as a call: the reference's
 * plane_dict is a host dict. */
int adsb_planes(adsb_ctx* ctx, adsb_decoded* rows, int32_t cap, int32_t* n_out);
int adsb_stream_planes(adsb_ctx* ctx, const int32_t* streams, int32_t n_sel, adsb_decoded* rows, int32_t cap, int32_t* first,
                       int32_t* n_out);
/* PLANE AGES (ADSB_FLAG_PLANE_AGES): plane_dict's last_seen on the device, and expiry by it.  update_plane sets
 * last_seen = int(time.time()) (decoder.py:424,433); with the decoder's clock of ADSB_FLAG_DECODE that is
 * (long long)timestamp of the PDU, and last_seen moves exactly where num_msgs moves.  After a call a plane's last_seen is the
 * clock of the last PDU of the call, in publication order, that reached update_plane for it -- the last one, not the
 * largest: adsb_decode_pdus may be given timestamps that go backwards.
 * adsb_planes_seen / adsb_stream_planes_seen are adsb_planes / adsb_stream_planes with one more output: last_seen[j] belongs
 * to rows[j] (cap entries each).  Rows, order, first[], the -ENOSPC count query, -EBUSY, the ordering behind the last decode
 * step and "changes no state" are those of the plain calls, byte for byte; rows or last_seen may be NULL when only the other
 * is wanted.
 * adsb_planes_expire / adsb_stream_planes_expire remove every plane with last_seen < cutoff: with cutoff = now - timeout the
 * decoder's `now - last_seen > timeout` of print_planes (decoder.py:493, PLANE_TIMEOUT_S :259); last_seen == cutoff stays.
 * Removal is `del self.plane_dict[key]`, the sweep the decoder carries commented out (decoder.py:435-439): the plane is gone,
 * its address is announced no longer -- an address/parity reply to it is unknown again until a later reply announces it --
 * and the next reply that reaches update_plane starts a new entry (num_msgs 1, no callsign, NaN altimetry, no CPR frames).
 * CONTRACT: every record and row decoded after the call is byte-identical to what the reference decoder publishes after the
 * same keys were deleted from its plane_dict at the same point of the publication order (snapshots and ADSB_BURST_AP_KNOWN /
 * _AP_FEC included).  An address that is announced but holds no plane has no last_seen and is left alone.
 * adsb_stream_planes_expire: streams / n_sel as for adsb_stream_planes; cutoffs[i] belongs to the i-th selected stream
 * (streams do not share a clock); unselected streams lose nothing; adsb_stream_decoder_stats' planes stays exact.  The
 * store is rehashed into one of the same size (linear probing cannot delete in place); a reset stream's stale slots are
 * dropped in the same pass.  *n_removed (may be NULL) is the number of planes removed, of all selected streams together.
 * All four: -EINVAL without the flag; -EBUSY while submitted tickets are pending; ordered behind the last queued table or
 * decode step.  Expiry changes nothing but the removed planes: adsb_last_result, adsb_last_decoded,
 * adsb_stream_last_decoded, framer and stream state are untouched, and a call that removes nothing changes no later byte.
 * ADSB_ABI_VERSION is unchanged: a flag and entry points only. */
int adsb_planes_seen(adsb_ctx* ctx, adsb_decoded* rows, int64_t* last_seen, int32_t cap, int32_t* n_out);
int adsb_stream_planes_seen(adsb_ctx* ctx, const int32_t* streams, int32_t n_sel, adsb_decoded* rows, int64_t* last_seen,
                            int32_t cap, int32_t* first, int32_t* n_out);
int adsb_planes_expire(adsb_ctx* ctx, int64_t cutoff, int64_t* n_removed);
int adsb_stream_planes_expire(adsb_ctx* ctx, const int32_t* streams, int32_t n_sel, const int64_t* cutoffs, int64_t* n_removed);
/* MERGED PICTURE: the fleet's per-receiver plane_dicts folded into one table on the device -- what one decoder feeding one
 * map shows (web/webserver.py reads one plane_dict), for a fleet whose receivers each hear a part of every aircraft.  The
 * context must have ADSB_FLAG_STREAM_DECODE | ADSB_FLAG_PLANE_AGES and open streams (-EINVAL otherwise: the rule needs
 * last_seen).  streams / n_sel as for adsb_stream_planes: NULL selects all streams, otherwise strictly ascending indices in
 * range (-EINVAL).  -EBUSY while submitted tickets are pending; ordered behind the last queued decode step.
 * A CONTRIBUTING entry is a live plane of a selected stream's current generation with last_seen >= cutoff: a reset stream's
 * stale slots and expired planes never contribute, cutoff = INT64_MIN hides nothing.  The cutoff only hides entries; nothing
 * is removed.  One cutoff for all selected streams presumes that their clocks are comparable, which they are when
 * adsb_stream_set_start was given real times.
 * Output: one row per distinct address with at least one contributing entry, in ascending address order.  rows[j] is a
 * snapshot row as adsb_stream_planes writes it (port ADSB_DEC_NONE, df 0, bits and pad bytes zero, icao the address);
 * info[j] belongs to rows[j].  num_msgs is the uint32 sum over the contributing entries: it wraps modulo 2^32.
 * info[j].last_seen is the largest last_seen among them, n_streams their number.
 * Four field groups are merged, each on its own: callsign (ADSB_DEC_HAS_CALLSIGN), altitude (ADSB_DEC_HAS_ALTITUDE), velocity
 * (ADSB_DEC_HAS_VELOCITY: velocity_we, velocity_sn and vertical_rate together) and position (latitude is not NaN: latitude
 * and longitude together).  A group is copied, byte for byte, from the contributing entry that has it and has the greatest
 * last_seen; ties go to the lowest stream index; src_* names that stream.  A group no contributing entry has is shown as an
 * empty plane shows it (flag clear, zero callsign / altitude / velocity, NaN position) with src_* = -1.  present is
 * ADSB_DEC_HAS_PLANE plus the flags of the groups found.  last_seen is per plane, not per field: the rule is "the freshest
 * entry that has the field", not a claim about the field's own age.
 * cap smaller than the number of rows is -ENOSPC with *n_out = the number needed and nothing written;
 * rows == NULL && info == NULL && cap == 0 is a count query; either of rows and info may be NULL when only the other is
 * wanted.  An empty result returns 0 with *n_out = 0.  The call changes no state: two merged calls with nothing between
 * them are byte-identical, adsb_stream_planes_seen before and after is byte-identical, and rows decoded afterwards are
 * byte-identical to rows decoded without it.  With one selected stream and cutoff = INT64_MIN the rows are those of
 * adsb_stream_planes_seen of that stream, info.last_seen its last_seen, n_streams 1 and every src_* that stream or -1.
 * CPR frames are not merged across receivers.  ADSB_ABI_VERSION is unchanged: an entry point only. */
typedef struct adsb_merged {      /* 32 bytes; info[j] belongs to rows[j] */
  int64_t last_seen;              /* the largest last_seen among the contributing streams */
  int32_t n_streams;              /* how many contributing streams hold this aircraft (>= 1) */
  int32_t src_callsign;           /* the stream each field group was taken from; -1: no contributing stream has it */
  int32_t src_altitude;
  int32_t src_velocity;
  int32_t src_position;
  int32_t pad;                    /* 0 */
} adsb_merged;
int adsb_stream_planes_merged(adsb_ctx* ctx, const int32_t* streams, int32_t n_sel, int64_t cutoff,
                              adsb_decoded* rows, adsb_merged* info, int32_t cap, int32_t* n_out);
/* Device memory on the context's device for callers that do not link HIP (a C or ctypes client of the *_device entry
 * points): hipMalloc / hipFree / a blocking hipMemcpy host -> device.  16-byte alignment is guaranteed.  No reference
 * counterpart (the reference never leaves host memory). */
int adsb_device_alloc(adsb_ctx* ctx, void** d, size_t bytes);
int adsb_device_free(adsb_ctx* ctx, void* d);
int adsb_device_upload(adsb_ctx* ctx, void* d, const void* host, size_t bytes);
/* eob_in = (offset of the last burst kept before this shard) + 63*sps, or a very negative number for the
 * first shard.  Compacts recs in place to the exact kept list; -EAGAIN if the head region was too short
 * (call adsb_shard_device again with a larger head_cands, or with 0 and adsb_stitch). */
int adsb_shard_fixup(adsb_burst* recs, int32_t n, int sps, int64_t eob_in, int32_t* n_kept);
/* Host stitch: cands = shard outputs concatenated in stream order; applies the re-trigger gate
 * (framer.py:121-123,165) in place (sets KEPT) and compacts the kept bursts to the front. */
int adsb_stitch(adsb_burst* cands, int32_t n, int sps, int32_t* n_kept);

/* 10*log10(peak/median) + 1.6 in float32 (framer.py:157) with libm's log10f.  NumPy's float32 log10 is
 * a SIMD routine on some hosts, so the reference's SNR bits are host dependent; the Python shim finalises
 * SNR with NumPy from (peak, median) -- those two ARE bit exact -- and this helper is for C callers. */
float adsb_snr_db(float peak, float median);

/* Host helper for the address/parity formats (DF 0/4/5/16/20/21/24), whose check needs the consumer's
 * aircraft table: returns crc(bits[0:L-24]) ^ bits[L-24:L] -- the announced address `aa` of
 * decoder.py:577,647 (0 for a clean DF 11/17/18/19) -- for the DF's length L; *df = downlink format,
 * *nbits = 56 / 112, or 0 for a DF check_parity() does not know (the 56-bit reading is returned).
 * Pure host arithmetic on one 14-byte payload; out pointers may be NULL. */
uint32_t adsb_mode_s_syndrome(const uint8_t bits[14], int32_t* df, int32_t* nbits);

/* The rule of ADSB_FLAG_FEC_CONSERVATIVE for one 14-byte payload of a demodulated burst, as plain host arithmetic: the
 * decoder's correct_burst_errors() (decoder.py:304-323 table, :738-763 lookup) for DF 11/17/18/19 with a non-zero syndrome,
 * the pattern looked up by its 25-bit compute_crc_2 key.  Returns the flags the device gives the record: the pre-filter bits
 * (ADSB_BURST_PARITY_OK / _LONG / _KNOWN_DF / DF) of out, plus ADSB_BURST_FEC_FIXED or ADSB_BURST_FEC_DF.  out = the repaired
 * payload when FEC_FIXED, else a copy of in (in and out may be the same array).  *first_bit / *nflip = the table's pattern
 * (bits first_bit .. first_bit+nflip-1) on a hit, FEC_DF included; -1 / 0 without one.  Out pointers may be NULL. */
uint32_t adsb_mode_s_fec(const uint8_t in[14], uint8_t out[14], int32_t* first_bit, int32_t* nflip);

/* ---- SOFT REPAIR (ADSB_FLAG_FEC_SOFT) ----------------------------------------------------------------------------------
 * WHICH RECORDS.  A record with ADSB_BURST_DEMOD and DF 11/17/18/19, without ADSB_BURST_PARITY_OK and without
 * ADSB_BURST_FEC_DF: its syndrome S = crc(bits[0:L-24]) ^ bits[L-24:L] is non-zero; L = 56 for DF 11, else 112.  The soft
 * repair runs AFTER the Conservative repair where the context has both, so ADSB_FLAG_FEC_CONSERVATIVE repairs exactly the
 * records it repairs alone.
 * WEAKNESS OF BIT i.  x1, x0 = the two samples adsb_last_confidence's ratio is made of, in the input's own format, converted
 * as everywhere.  hi = x1 > x0 ? x1 : x0, lo = x1 > x0 ? x0 : x1 (the slicer's own comparison).  key = lo / hi, ONE IEEE
 * float32 division (NumPy's float32 division gives the same bits), if hi > 0 && lo >= 0 && hi < +inf; otherwise 1.0f when
 * !(hi > 0) and 0.0f in the remaining cases.  A larger key is a weaker bit.
 * CANDIDATES.  Bits 5 .. L-1 with key >= min_key (bits 0-4 never: a soft repair changes neither the DF nor the length),
 * sorted by key descending, ties to the lower bit index; the first n_weak are kept, rank 0 the weakest.
 * SEARCH.  The non-empty subsets of the kept candidates with at most max_flips members; a subset matches when the XOR of
 * its members' syndromes (bit i: x^(L-1-i) mod G) equals S.  Among the matches the fewest flips win, among those the
 * smallest mask (mask bit k = rank k).  Integers only: no float sums, no dependence on any order of evaluation.
 * ON A MATCH.  The bits are flipped, the pre-filter bits recomputed as the Conservative repair does, ADSB_BURST_FEC_FIXED
 * set.  All 16 bits of adsb_burst.flags are taken: what tells a soft repair from a Conservative one is the record's
 * adsb_soft_fix row (adsb_last_soft): nflip != 0.  A record the rule does not apply to has an all-zero row; one it applies
 * to has ncand = the candidates kept and bit[] = the flipped bits ascending, padded with 0xFF.
 * FALSE REPAIRS (derived, not measured).  A reply of random bits has a uniformly random 24-bit syndrome, and T = sum over
 * k = 1..max_flips of C(n_weak, k) subsets are tried: it is "repaired" with probability about T / 2^24 -- T = 92: 5.5e-6 at
 * the defaults (8, 3); T = 6884: 4.1e-4 at the caps (16, 5).  The Mode S CRC has codewords of weight 6, so two different
 * 3-bit subsets can match the same syndrome: the tie rule above then decides.
 * IN A BATCH (ADSB_FLAG_FEC_SOFT_BATCH).  Item i's records and rows of adsb_process_batch* are those of adsb_process_format on an
 * ADSB_FLAG_FEC_SOFT context with the same rule and the same Conservative flag, over item i's samples at its threshold: a
 * record's samples are its own item's, never a neighbour's.  A stream's records and rows over all adsb_process_stream_batch*
 * calls are those of ONE such call over the concatenated chunks, with the existing stream-batch deviations; a repair changes
 * neither offset, DF nor length, so what a stream carries from call to call is what it carries without the flag.  Items the
 * library runs through its ordinary pass (longer than ADSB_BATCH_ITEM_MAX, or with overflowed lists) are repaired there; their
 * records and rows take the item's place.  In a fleet the derived false-repair odds above hold PER HEARING: a false repair
 * produces an essentially random payload, which joins another receiver's group (de-duplication, multilateration) only if it
 * equals that receiver's payload within the window -- another factor of about 2^-88 for a long reply -- so it can feed no
 * multilateration fix; it can still touch its own address's plane in the decoder, exactly as on one receiver.
 * OUT OF SCOPE.  The address/parity formats (DF 0/4/5/16/20/21/24): their syndrome is the address, and the verdict needs the
 * aircraft table. */
typedef struct adsb_soft_fix { /* 8 bytes */
  uint8_t nflip;  /* 0: not repaired by this rule */
  uint8_t ncand;  /* candidates kept (<= n_weak); 0 in the row of a record the rule does not apply to */
  uint8_t bit[5]; /* the flipped bits, ascending, padded with 0xFF */
  uint8_t pad;
} adsb_soft_fix;
typedef struct adsb_soft_fec_rule { /* 16 bytes */
  int32_t n_weak;    /* 1 .. 16, default 8 */
  int32_t max_flips; /* 1 .. 5, default 3 */
  float min_key;     /* 0 .. 1, default 0 */
  uint32_t flags;    /* 0 */
} adsb_soft_fec_rule;
/* ADSB_FLAG_FEC_SOFT and ADSB_FLAG_FEC_SOFT_BATCH contexts.  -EINVAL for a value outside the ranges above, a NaN min_key or flags != 0; -EBUSY while
 * tickets are pending.  The rule holds for every call queued afterwards. */
int adsb_set_soft_fec(adsb_ctx* ctx, const adsb_soft_fec_rule* rule);
/* *rows -> n adsb_soft_fix in the context's pinned memory: row t belongs to record t of the last finished call (blocking
 * call or adsb_wait), or to tag t of the last adsb_demod_work.  Valid until the next call on the context. */
int adsb_last_soft(adsb_ctx* ctx, const adsb_soft_fix** rows, int32_t* n);
/* ADSB_FLAG_FEC_SOFT_BATCH contexts (-EINVAL otherwise).  *rows -> n adsb_soft_fix in the context's memory: row t belongs to
 * out[t] of the last adsb_process_batch* / adsb_process_stream_batch* call that delivered its records (n = 0 before the first).
 * Valid until the next call on the context.  adsb_last_soft and adsb_last_result stay what they are. */
int adsb_batch_last_soft(adsb_ctx* ctx, const adsb_soft_fix** rows, int32_t* n);
/* The rule for one 14-byte payload of a demodulated burst as plain host arithmetic, beside adsb_mode_s_fec: key[i] = the
 * weakness of bit i (a NaN key is no candidate), rule = NULL: the defaults (n_weak and max_flips beyond their caps count as
 * the caps).  Returns the pre-filter bits of out, plus ADSB_BURST_FEC_FIXED on a match; out = the repaired payload then, else a
 * copy of in.  *fix = the row.  out and fix may be NULL. */
uint32_t adsb_mode_s_soft_fec(const uint8_t in[14], const float key[112], const adsb_soft_fec_rule* rule, uint8_t out[14],
                              adsb_soft_fix* fix);

/* The per-PDU rule of ADSB_FLAG_AIRCRAFT_TABLE for one 14-byte payload of a demodulated burst, as plain host arithmetic
 * (fec != 0: the context also has ADSB_FLAG_FEC_CONSERVATIVE).  *aa = the AA of an AP-format reply, else -1.  *announce = the
 * address the reply announces whatever the table holds (DF 11, and DF 17 / 18 with CF 0,1,6 / 19 with AF 0 of TC 1-4, 9-18
 * or 19 with ST 1,2, after the parity check and, with fec, the decoder's repair), else -1.  Returns ADSB_BURST_AP_FEC when
 * fec and an AP reply whose AA is unknown would be accepted by the decoder's repair (its (AA, last bit) is one of the error
 * patterns); *fec_announce = what that reply then announces -- the pre-repair AA when the repaired DF is 0/4/5/16/20/21,
 * the repaired reply's address by the rule above when it became DF 11/17/18/19, -1 otherwise (or without the repair).
 * Out pointers may be NULL. */
uint32_t adsb_mode_s_aircraft(const uint8_t bits[14], int32_t fec, int32_t* aa, int32_t* announce, int32_t* fec_announce);

/* How one call over n_samples is cut on a device that keeps `resident_wavefronts` wavefronts of the streaming kernel
 * resident (adsb_stats.detect_grid / blocks_per_cu tell what a context uses: CUs x blocks_per_cu x 4, or x 1 for the 8-bit formats): *units chunks of
 * *samples_per_chunk samples each (the last may be shorter), one wavefront and one output list per chunk.  One resident
 * round is the floor; a bulk call runs up to eight rounds of shorter chunks (never shorter than 4096 samples) so that the
 * dispatcher evens out wavefronts that finish apart.  Pure host arithmetic (no device needed), the reference has no
 * counterpart: framer.py:83-174 walks the whole in0 in one Python loop.  Returns 0 or -EINVAL. */
int32_t adsb_plan_chunks(int64_t n_samples, int64_t resident_wavefronts, int64_t* units, int64_t* samples_per_chunk);

int adsb_get_stats(adsb_ctx* ctx, adsb_stats* out);
int adsb_reset_stats(adsb_ctx* ctx);
/* The duration (ms, HIP events on the compute stream) of every k_detect launch the context has timed since the last
 * adsb_reset_stats, oldest first -- the last 4096 of them; contexts created with ADSB_FLAG_TIMING only.  adsb_stats holds
 * their sum; this is the per-launch sequence (measurement aid: tools/launch_hist.py holds it against a rocprofv3 kernel
 * trace launch by launch).  No reference counterpart.  *n = durations written (<= cap). */
int adsb_detect_history(adsb_ctx* ctx, float* ms, int32_t cap, int32_t* n);
/* Text of the last error on this context ("" if none). */
const char* adsb_last_error(adsb_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* ADSB_HIP_H */
