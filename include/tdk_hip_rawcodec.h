/*
 * tdk_hip_rawcodec.h -- lossless compression of raw mosaics on the device (libtdk_hip.so).  tdk_rawcodec_encode turns a raw frame
 * (uint16 codes, or the 12-bit packed bytes of tdk_hip.h in either nibble order) into a self-describing byte stream,
 * tdk_rawcodec_decode turns the stream back into uint16 codes, packed bytes or the float mosaic of tdk_decode12_f32 / _f16.  Every
 * uint16 value survives the round trip.  The reference has no counterpart: its only raw container is the packed form, 1.5 bytes a site.
 *
 * include/tdk_hip.h (the reference's surface) and the other tdk_hip_*.h headers stay pinned; the codec is declared here, with its own
 * version number.  The conventions of tdk_hip.h apply: device pointers, a HIP stream per call, TDK_OK or a tdk_status code with the
 * message in tdk_last_error(), nothing allocates device memory.  Formats are the TDK_RAW_* values of tdk_hip_raw.h.
 *
 * This header is the normative text of the format; tests/rawcodec_spec.py restates it in NumPy.
 *
 * ---- The format "TDKR", version 1.  Everything is little-endian and every section starts 4-byte aligned.
 *
 * Geometry.  The frame is W x H sites, 1 <= W, H <= 65535 and W*H <= 2^30.  A span is 64 consecutive sites of one row (the last span
 * of a row may be shorter), S = ceil(W/64).  A segment is 8 consecutive spans, 512 sites (the last segment of a row may be shorter),
 * G = ceil(W/512).  The format knows no Bayer pattern, only that same-colour neighbours are two sites apart in a row.
 *
 * Prediction chain.  For a segment (y, g) and a parity p in {0, 1} the sequence is v_k = sample[y][512*g + 2*k + p] while that site
 * exists.  anchor = v_0, or 0 for an empty sequence.  d_0 = 0; for k >= 1, d_k = (v_k - v_(k-1)) mod 2^16, read as int16 t;
 *   z = ((t << 1) ^ (t >> 15)) & 0xFFFF                         (zigzag: 0, -1, 1, -2, ... -> 0, 1, 2, 3, ...)
 *
 * Groups and payload.  A group (y, span, p) is the 32 values z_k of that span and parity: sample i of the group is the site
 * 64*span + 2*i + p; sites past W count as z = 0.  Its width b is the bit length of the largest z, 0..16.  Its payload is b 32-bit
 * words: word j carries bit j of z of the group's i-th sample in bit i -- bit planes.  A segment's payload is its groups in order, span
 * ascending, parity 0 then 1; segments follow row-major, y then g.
 *
 * Stream layout.
 *   header, 32 bytes   'T' 'D' 'K' 'R', u16 version = 1, u16 bits, u32 width, u32 height, u32 payload_words, u32 total_bytes,
 *                      u32 flags = 0, u32 reserved = 0.  bits is informational, 1..16; 12 for packed input.
 *   anchors            u16[H][G][2]
 *   offsets            u32[H][G]: the word index of the segment's payload from the payload start, an exclusive prefix sum
 *   widths             u8[H][S][2], zero-padded to a multiple of 4
 *   payload            u32[payload_words]
 * Sizes:  table_bytes = 32 + 8*H*G + round4(2*H*S);   total_bytes = table_bytes + 4*payload_words;
 *         max_stream_bytes = table_bytes + 4*16*2*H*S.
 * The tables cost 0.375 bit per site (the offsets 0.06 of that); a constant frame encodes to exactly table_bytes.
 *
 * Why this shape.  Groups of 32 make every payload whole words; a 64-lane ballot produces the plane words of two groups at once; the
 * chain through a segment is a wave-wide prefix sum on decode; the offset table lets the decoder run as one launch without a scan.
 *
 * ---- Decoding.  A segment's samples are v_0 = anchor, v_k = (anchor + t_1 + ... + t_k) mod 2^16 with t = (z >> 1) ^ -(z & 1): the encoder
 * writes z_0 = 0, and a decoder does not look at it.  Outputs (out_format):
 *   TDK_RAW_U16                           (height, width) uint16
 *   TDK_RAW_PACKED12, TDK_RAW_PACKED12_IDS   the bytes tdk_decode12_u16 reads the decoded samples from, a sample above 4095 taken as 4095:
 *                                         for the standard order the bytes of tdk_encode12_u16.  For the IDS order tdk_encode12_u16 puts
 *                                         the two low nibbles the other way round than tdk_decode12_u16 reads them (as the reference has
 *                                         it); the codec follows the decoder, b2 = ((p1 & 15) << 4) | (p0 & 15), so that a packed frame
 *                                         comes back byte for byte in either order
 *   TDK_RAW_F32, TDK_RAW_F16              the bits of tdk_decode12_f32 / tdk_decode12_f16 with scaled on: (float)sample * (1.0f / 4095.0f),
 *                                         rounded once more for binary16
 * The packed forms, as input and as output, need an even number of sites, width*height: a packed buffer knows no rows, two sites share
 * three bytes.  With an odd width a pair reaches from one row, or one segment, into the next; its three bytes are then written by the wave
 * of its first site alone, which takes the second sample from the anchor of the segment that follows, after checking that segment's tables.
 *
 * Validation happens on the device; *status is written by every call:
 *   TDK_RAWCODEC_BAD_MAGIC (bit 0)    magic or version wrong
 *   TDK_RAWCODEC_BAD_SIZE (bit 1)     width or height of the header differ from the call's
 *   TDK_RAWCODEC_BAD_TABLES (bit 2)   some segment's tables or payload pass data_bytes, or a width byte is above 16
 * With bit 0 or bit 1 set the whole output is zero (and bit 2 is not looked at: the tables have no known place).  With bit 2 set the
 * offending segments are zero -- all of them when the tables themselves pass data_bytes.  No load or store outside [data, data +
 * data_bytes) and the output happens, whatever the stream holds: every table index comes from the call's width and height, and an
 * offset is used only after offset + count has been held against data_bytes.
 *
 * ---- Kernels (csrc/rawcodec.hip), wave64, one wave per segment, four steps of 128 sites; lane i holds sites 2i and 2i+1 of a step, so
 * the left same-parity neighbour is the lane before, with a carry between steps.  Encode is three launches: measure (anchors, width
 * bytes, and the segment's word count into its slot of offsets), scan (one workgroup: counts -> exclusive prefix sum in place, the
 * header, the padding of widths, *length), pack (recomputes z, forms plane words by ballot: the low half belongs to lanes 0..31, the
 * high half to lanes 32..63; a segment whose payload would pass capacity is skipped).  Decode is one launch: a wave stages its
 * payload (at most 1 KB) in LDS, each lane rebuilds z from its group's b words, undoes the zigzag and takes part in a wave-wide
 * inclusive scan; one extra workgroup reads all tables and writes *status, so that no atomic is needed.
 *
 * No workspace, no atomics on global memory, no memset, no copy, no synchronisation: both directions are capturable in a graph from the
 * first call, and bit-reproducible.  *length (int64) and *status (int32) stay in device memory.
 */
#ifndef TDK_HIP_RAWCODEC_H
#define TDK_HIP_RAWCODEC_H

#include <stddef.h>
#include <stdint.h>

#include "tdk_hip.h"
#include "tdk_hip_raw.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_RAWCODEC_ABI_VERSION 1

#define TDK_RAWCODEC_FORMAT_VERSION 1
#define TDK_RAWCODEC_HEADER_BYTES 32
#define TDK_RAWCODEC_SPAN 64         /* sites of a span: two groups of 32 */
#define TDK_RAWCODEC_SEGMENT 512     /* sites of a segment: the reach of one prediction chain, the work of one wave */
#define TDK_RAWCODEC_MAX_SITES 1073741824   /* 2^30 */

/* bits of *status of tdk_rawcodec_decode */
#define TDK_RAWCODEC_BAD_MAGIC 1
#define TDK_RAWCODEC_BAD_SIZE 2
#define TDK_RAWCODEC_BAD_TABLES 4

int tdk_rawcodec_abi_version(void);

/* Bytes of header, anchors, offsets and widths: the length of the stream of a constant frame.  0 for a size the codec rejects. */
size_t tdk_rawcodec_table_bytes(int width, int height);

/* A capacity every stream of this size fits in: every group at 16 bits.  0 for a size the codec rejects. */
size_t tdk_rawcodec_max_stream_bytes(int width, int height);

/* Three launches on `stream`.  src: (height, width) uint16 for TDK_RAW_U16, width*height*3/2 packed bytes for TDK_RAW_PACKED12 /
 * TDK_RAW_PACKED12_IDS (width*height even, bits = 12; the samples are those of tdk_decode12_u16).  data: `capacity` bytes, 4-byte aligned,
 * capacity >= tdk_rawcodec_table_bytes (the tables always fit).  *length: total_bytes, or -1 when the payload does not fit in
 * capacity; nothing at or behind data + capacity is written either way.  Argument errors (null pointers, format, sizes, bits,
 * alignment, capacity, overlap of data or length with src and with each other) are reported before any HIP call. */
int tdk_rawcodec_encode(const void* src, int src_format, int width, int height, int bits, void* data, size_t capacity, int64_t* length,
                        tdk_stream_t stream);

/* One launch on `stream`.  data: data_bytes >= 32 bytes, 4-byte aligned (a stream read from a file: its whole length).  out: the frame
 * in out_format, at the alignment of its element type.  *status: see above.  Argument errors (null pointers, format, sizes,
 * alignment, data_bytes, overlap of out or status with data and with each other) are reported before any HIP call. */
int tdk_rawcodec_decode(const void* data, size_t data_bytes, void* out, int out_format, int width, int height, int* status, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
