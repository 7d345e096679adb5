/*
 * tdk_hip_ext.h -- entry points of libtdk_hip.so beyond the reference's surface.
 *
 * include/tdk_hip.h mirrors the reference's extension.cpp op for op and stays pinned; what the library offers on top of that is
 * declared here, with its own version number.  The conventions of tdk_hip.h apply: device pointers unless named host_*, a HIP
 * stream per call, TDK_OK or a tdk_status code with the message in tdk_last_error(), nothing allocates device memory.
 */
#ifndef TDK_HIP_EXT_H
#define TDK_HIP_EXT_H

#include "tdk_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDK_EXT_ABI_VERSION 1

int tdk_ext_abi_version(void);

/* ---- Device-resident JPEG encode: the encoder of tdk_jpeg_encode (csrc/jpeg.hip) without a single host round trip.  The
 * optimal Huffman tables (T.81 K.2 / K.3) are built on the device from the scan's histograms, the markers (frame header, DHT,
 * SOS, EOI) are written by the device at a stream position kept in the workspace, and the stuffed scans go straight into `out`.
 * The call only enqueues work -- no synchronisation, no allocation, no copy from host memory -- so it can be captured in a graph.
 * The bytes are those of tdk_jpeg_encode for the same arguments.
 *   image, width, height, input_format, subsampling, progressive: as tdk_jpeg_encode; quality must be 1..100 (no clamping).
 *   workspace: tdk_jpeg_device_workspace_bytes(), 256-byte aligned.
 *   out, out_capacity: the stream's destination (out may be NULL when out_capacity is 0).  Nothing is ever written at or beyond
 *   out + out_capacity.
 *   length_dev: one int64 on the device, 8-byte aligned: the stream's length once the work has run, or -1 when it did not fit in
 *   out_capacity (the contents of `out` are then undefined, but nothing beyond the capacity was touched).
 * tdk_jpeg_device_max_stream_bytes(): a capacity every stream of that geometry fits in (the stream region of tdk_jpeg_encode).
 * Both size queries run on the host and return 0 for an invalid geometry. */
size_t tdk_jpeg_device_workspace_bytes(int width, int height, int subsampling);
size_t tdk_jpeg_device_max_stream_bytes(int width, int height, int subsampling, int progressive);
int tdk_jpeg_encode_device(const void* image, int width, int height, int input_format, int quality, int subsampling, int progressive,
                           void* workspace, uint8_t* out, size_t out_capacity, int64_t* length_dev, tdk_stream_t stream);

/* test hook: the optimal tables of `ntables` histograms (256 uint32 counts each) as the device encoder builds them.  Per table
 * bits_vals_dev receives BITS[16] (the number of codes of length 1..16) then HUFFVAL[256] (zero-padded), packed_dev 256 uint32 of
 * code << 8 | length (0 for a symbol without a code). */
int tdk_jpeg_huffman_tables(const uint32_t* counts_dev, int ntables, uint8_t* bits_vals_dev, uint32_t* packed_dev, tdk_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
