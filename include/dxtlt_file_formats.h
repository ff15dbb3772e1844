/*
 * dxtlt_file_formats.h -- the callers on the file side of the hot path: the 4-byte
 * TransformHeader that records how a texture was transformed, and the DDS container handler that uses it.
 * Host-side byte bookkeeping only; the payload itself goes through the gfx950 path (dxtlt_gfx950.h).
 *
 * Reference (paths under /root/reference/src/):
 *   TransformHeader      api/dxt-lossless-transform-file-formats-api/src/embed/mod.rs:105-162
 *                        u32 little-endian: bits 0-3 format, bits 4-31 format data
 *   TransformFormat      .../embed/transform_format.rs:10-31     Bc1=0 Bc2=1 Bc3=2 Bc7=3 Bc6H=4 ...
 *   BC1 / BC2 data       .../embed/formats/bc1.rs:34-82, bc2.rs   version:2 | split_colour:1 | variant:2
 *                        (variant Variant1=0 Variant2=1 Variant3=2 None=3), other bits zero
 *   BC3 data             .../embed/formats/bc3.rs:28-43           upstream: version bits only (placeholder, and
 *                        dispatch refuses BC3).  ADDITIVE here: split_alpha at bit 2, split_colour at bit 3,
 *                        variant at bits 4-5, so that BC3 files written by this build can be restored by it.
 *   DDS parsing          extensions/file-formats/dxt-lossless-transform-dds/src/dds/parse_dds.rs:58-330
 *   C exports            .../dds/exports.rs:12 (is_dds), :39 (parse_dds)
 *   DDS handler          .../handler/file_format_handler.rs:16-135  (copy header, transform payload, copy the
 *                        leftover bytes, overwrite the 'DDS ' magic with the TransformHeader; inverse restores it)
 */
#ifndef DXTLT_FILE_FORMATS_H
#define DXTLT_FILE_FORMATS_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#include "dlt_size_estimator.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DXTLT_TRANSFORM_HEADER_SIZE 4

/* TransformFormat codes (transform_format.rs:10-31) */
#define DXTLT_TF_BC1 0
#define DXTLT_TF_BC2 1
#define DXTLT_TF_BC3 2
#define DXTLT_TF_BC7 3
/* codes upstream has reserved header layouts for, without a transform behind them yet */
#define DXTLT_TF_BC6H 4
#define DXTLT_TF_RGBA8888 5
#define DXTLT_TF_BGRA8888 6
#define DXTLT_TF_BGR888 7
#define DXTLT_TF_BC4 8
#define DXTLT_TF_BC5 9

/* embed/mod.rs:96-103: bytes a file format must reserve beyond the 4-byte header for these two */
#define DXTLT_BC7_ADDITIONAL_SPACE 48
#define DXTLT_BC6H_ADDITIONAL_SPACE 80

/* status codes of this header's functions */
#define DXTLT_FF_OK 0
#define DXTLT_FF_OUTPUT_TOO_SMALL 1          /* FormatHandlerError::OutputBufferTooSmall */
#define DXTLT_FF_INVALID_INPUT_HEADER 2      /* FormatHandlerError::InvalidInputFileHeader / InvalidRestoredFileHeader */
#define DXTLT_FF_INPUT_TOO_SHORT 3           /* InputTooShort / InputTooShortForStatedTextureSize */
#define DXTLT_FF_UNKNOWN_TRANSFORM_FORMAT 4  /* TransformError::UnknownTransformFormat (not BC1/BC2/BC3) */
#define DXTLT_FF_CORRUPTED_EMBEDDED_DATA 5   /* EmbedError::CorruptedEmbeddedData */
#define DXTLT_FF_INVALID_DATA_ALIGNMENT 6    /* TransformError::InvalidDataAlignment */
#define DXTLT_FF_TRANSFORM_FAILED 7          /* the device path failed; see dxtlt_last_error() */
#define DXTLT_FF_ESTIMATOR_FAILED 8          /* auto mode: estimator callback error */
#define DXTLT_FF_NULL_POINTER 9

/* Pack / unpack a TransformHeader value.  `decorrelation_mode` uses the CORE numbering (None=0, Variant1..3). */
uint32_t dxtlt_transform_header_pack(int32_t transform_format, uint8_t decorrelation_mode,
                                     bool split_alpha_endpoints, bool split_colour_endpoints);
int32_t dxtlt_transform_header_unpack(uint32_t header, int32_t *transform_format, uint8_t *decorrelation_mode,
                                      bool *split_alpha_endpoints, bool *split_colour_endpoints);

/* TransformHeader itself (embed/mod.rs:105-140): format code in bits 0-3, format-specific data in bits 4-31, stored as a
 * little-endian u32.  _new masks `format_data` to 28 bits; _format returns the code, or -1 for one this version does not know
 * (TransformFormat::from_u8 -> None: 10 ... 15), so that files written by later versions are refused, not misread. */
uint32_t dxtlt_transform_header_new(int32_t transform_format, uint32_t format_data);
int32_t dxtlt_transform_header_format(uint32_t header);
uint32_t dxtlt_transform_header_format_data(uint32_t header);
void dxtlt_transform_header_write(uint32_t header, uint8_t *ptr);   /* 4 bytes, little endian */
uint32_t dxtlt_transform_header_read(const uint8_t *ptr);

/* Header data of the formats upstream keeps placeholders for (embed/formats/bc4.rs, bc5.rs: `split_endpoints`; rgba8888.rs,
 * bgra8888.rs, bgr888.rs: `decorrelation`): version:2 (only 0 valid) | flag:1 | reserved:25 (must be zero).  No transform
 * exists for them upstream; this build's own (BC4 / BC5 and the pixel formats, behind the opt-in switches below) write
 * tagged words that these two functions do not produce and refuse.  With the switches off the DDS calls answer
 * DXTLT_FF_UNKNOWN_TRANSFORM_FORMAT -- but a tool that walks headers can name them.  _unpack: DXTLT_FF_UNKNOWN_TRANSFORM_FORMAT for any other format code,
 * DXTLT_FF_CORRUPTED_EMBEDDED_DATA for another version or non-zero reserved bits. */
uint32_t dxtlt_transform_header_pack_reserved_format(int32_t transform_format, bool flag);
int32_t dxtlt_transform_header_unpack_reserved_format(uint32_t header, int32_t *transform_format, bool *flag);

/* DdsFormat (parse_dds.rs:6-20), #[repr(u8)] */
enum DdsFormat
#ifdef __cplusplus
  : uint8_t
#endif
{
  NotADds = 0,
  Unknown = 1,
  BC1 = 2,
  BC2 = 3,
  BC3 = 4,
  BC6H = 5,
  BC7 = 6,
  RGBA8888 = 7,
  BGRA8888 = 8,
  BGR888 = 9,
  BC4 = 10,
  BC5 = 11,
};
#ifndef __cplusplus
typedef uint8_t DdsFormat;
#endif

/* parse_dds.rs:22-28, #[repr(C)] */
typedef struct DdsInfo {
  DdsFormat Format;
  uint8_t DataOffset;
  uint32_t DataLength;
} DdsInfo;

/* exports.rs:12 -- at least 128 bytes and the 'DDS ' magic */
bool is_dds(const uint8_t *ptr, size_t len);
/* exports.rs:39 -- {NotADds,0,0} when ptr is NULL, len is 0 or the data is not a DDS */
DdsInfo parse_dds(const uint8_t *ptr, size_t len);

/* DdsHandler::transform_bundle with a manual builder: copy the header, transform the BC1/BC2/BC3 payload with the
 * given settings on the GPU, copy any trailing bytes, replace the magic with the TransformHeader. */
int32_t dxtlt_dds_transform(const uint8_t *input, size_t input_len, uint8_t *output, size_t output_len,
                            uint8_t decorrelation_mode, bool split_alpha_endpoints, bool split_colour_endpoints);
/* Same with an auto builder: settings chosen by transform_bcN_auto with `estimator`. */
int32_t dxtlt_dds_transform_auto(const uint8_t *input, size_t input_len, uint8_t *output, size_t output_len,
                                 const DltSizeEstimator *estimator, bool use_all_decorrelation_modes);
/* DdsHandler::untransform: read the TransformHeader from the first 4 bytes, restore the magic, untransform. */
int32_t dxtlt_dds_untransform(const uint8_t *input, size_t input_len, uint8_t *output, size_t output_len);

/* ADDITIVE, off by default.  Upstream knows no BC7 transform and its dispatch refuses BC7 payloads
 * (handlers/dispatch.rs), which the three functions above reproduce (DXTLT_FF_UNKNOWN_TRANSFORM_FORMAT).  With this
 * switch on (process-wide), BC7 DDS payloads go through this build's own format (dxtlt_bc7.h, docs/BC7_FORMAT.md) and
 * the header carries TransformFormat::Bc7 = 3 (embed/transform_format.rs:18) with the 28 data bits set to a vendor
 * tag (0xD175, bits 27..12) and this build's format version (2, bits 11..0) -- never all zeros, which is what
 * upstream's own first BC7 header version would be; dxtlt_dds_untransform then accepts exactly that word.  Only this
 * build can read such files back. */
void dxtlt_file_formats_enable_bc7(bool enabled);

/* ADDITIVE, off by default (process-wide), like the BC7 switch.  Upstream parses BC6H DDS files (DXGI 94-96) but its handler
 * answers FormatNotImplemented(Bc6H); with this switch off the DDS calls refuse BC6H payloads
 * (DXTLT_FF_UNKNOWN_TRANSFORM_FORMAT) exactly as before.  With it on, dxtlt_dds_transform, _auto, _untransform and
 * dxtlt_dds_transform_batch take UF16, SF16 and typeless BC6H payloads through this build's own format (dxtlt_bc6h.h,
 * docs/BC6H_FORMAT.md; no settings, so _auto uses the one layout).  The header carries TransformFormat::Bc6H = 4 with the
 * BC7 scheme's data bits: vendor tag 0xD175 (bits 27..12) and layout version 1 (bits 11..0); dxtlt_dds_untransform accepts
 * exactly that word (else DXTLT_FF_CORRUPTED_EMBEDDED_DATA).  Only this build can read such files back. */
void dxtlt_file_formats_enable_bc6h(bool enabled);
/* The header word of a BC6H file written with this build's format. */
uint32_t dxtlt_transform_header_pack_bc6h(void);

/* ADDITIVE, off by default (process-wide), like the BC7 switch.  Upstream reserves TransformFormat::Bc4 = 8 / Bc5 = 9 and a
 * placeholder settings struct (embed/formats/bc4.rs, bc5.rs: split_endpoints) but defines no transform; with this switch off the
 * DDS calls refuse BC4 / BC5 payloads (DXTLT_FF_UNKNOWN_TRANSFORM_FORMAT) exactly as before.  With it on, dxtlt_dds_transform,
 * _auto, _untransform and dxtlt_dds_transform_batch take BC4 (ATI1, BC4U, BC4S, DXGI 79-81) and BC5 (ATI2, BC5U, BC5S, DXGI 82-84)
 * payloads through this build's layout (dxtlt_bc45.h, docs/BC45_FORMAT.md); `split_alpha_endpoints` carries split_endpoints and
 * the decorrelation mode and colour split are ignored.  The header's 28 data bits follow the BC7 precedent so that upstream never
 * misreads such a file: bits 0-1 upstream's placeholder version 0, bit 2 split_endpoints, bits 11..3 this build's layout version
 * (1), bits 27..12 the vendor tag 0xD175.  Upstream's unpack -- and dxtlt_transform_header_unpack_reserved_format -- reject the
 * word (its reserved bits are not zero); dxtlt_dds_untransform accepts exactly the two tagged words per format and nothing else
 * (DXTLT_FF_CORRUPTED_EMBEDDED_DATA).  Only this build can read such files back. */
void dxtlt_file_formats_enable_bc45(bool enabled);
/* The tagged header word of a BC4 (DXTLT_TF_BC4) or BC5 (DXTLT_TF_BC5) file written with this layout; 0 for any other code. */
uint32_t dxtlt_transform_header_pack_bc45(int32_t transform_format, bool split_endpoints);

/* ADDITIVE, off by default (process-wide), like the BC7 switch.  Upstream reserves TransformFormat::Rgba8888 = 5, Bgra8888 = 6 and
 * Bgr888 = 7 with a placeholder settings struct (embed/formats/rgba8888.rs, bgra8888.rs, bgr888.rs: decorrelation) but defines no
 * transform; with this switch off the DDS calls refuse these payloads and header codes (DXTLT_FF_UNKNOWN_TRANSFORM_FORMAT) exactly
 * as before.  With it on, dxtlt_dds_transform, _auto, _untransform and dxtlt_dds_transform_batch take RGBA8888 (DXGI 27-32, legacy
 * masks), BGRA8888 (DXGI 87, 90, 91, legacy masks) and BGR888 (legacy 24-bit masks) payloads through this build's layout
 * (dxtlt_pixels.h, docs/PIXEL_FORMAT.md).  The settings triple is read as the generic entry points read it for format codes 8 / 9:
 * decorrelation_mode != 0 is `decorrelate`; no colour split = INTERLEAVED, colour split alone = PLANAR, colour and alpha split =
 * PLANAR_DELTA.  _auto applies the fixed setting (decorrelate, PLANAR_DELTA) and never calls the estimator: the built-in estimator
 * ranks pixel layouts against what a compressor does with them (docs/PIXEL_FORMAT.md).  A payload length that is not a multiple
 * of the pixel size is DXTLT_FF_INVALID_DATA_ALIGNMENT.  The header's 28 data bits: bits 0-1 upstream's placeholder version 0, bit
 * 2 decorrelate, bits 4..3 the layout (0..2), bits 11..5 this build's layout version (1), bits 27..12 the vendor tag 0xD175.
 * Upstream's unpack -- and dxtlt_transform_header_unpack_reserved_format -- reject the word (its reserved bits are not zero);
 * dxtlt_dds_untransform accepts exactly the six tagged words per format code and nothing else (DXTLT_FF_CORRUPTED_EMBEDDED_DATA).
 * Only this build can read such files back. */
void dxtlt_file_formats_enable_pixels(bool enabled);
/* ADDITIVE, off by default (process-wide); means something only with dxtlt_file_formats_enable_pixels(true).  Off,
 * dxtlt_dds_transform_auto treats a pixel payload as described above: the fixed setting, the estimator never called.  On, the
 * payload goes through dxtlt_transform_pixels_auto (dxtlt_pixels.h) with the caller's estimator -- everything on the device for
 * dxtlt_builtin_entropy_estimator() (dxtlt_entropy_estimator.h), per candidate one download and one callback for any other --
 * and the header word records the setting it chose: one of the six tagged words, which dxtlt_dds_untransform reads back as ever. */
void dxtlt_file_formats_enable_pixel_auto(bool enabled);
/* The tagged header word of an RGBA8888 (5), BGRA8888 (6) or BGR888 (7) file written with this layout; 0 for any other code or
 * layout > 2. */
uint32_t dxtlt_transform_header_pack_pixels(int32_t transform_format, bool decorrelate, uint8_t layout);

/* ADDITIVE: many DDS files per call -- the file-after-file loop of the reference's CLI
 * (tools/dxt-lossless-transform-cli/src/commands/transform/mod.rs:154-199) over ONE pinned upload / launch / download
 * pipeline (dxtlt_transform_batch_host, dxtlt_gfx950.h) instead of a PCIe round trip per file.  Every item is checked
 * exactly like dxtlt_dds_transform / dxtlt_dds_untransform would check it and receives that call's status in `status`;
 * the items that pass are transformed together.  inverse = false: `decorrelation_mode` / `split_*` are the settings to
 * apply (as in dxtlt_dds_transform); inverse = true: the settings come from each file's TransformHeader and those fields
 * are ignored.  BC7 files (with the switch above on) ride in the same pipeline.  Returns the number of
 * items whose status is not DXTLT_FF_OK (0 = all done).  If the shared device pipeline fails, every item that was in it
 * gets DXTLT_FF_TRANSFORM_FAILED and its output is unspecified. */
typedef struct DxtltDdsBatchItem {
    const uint8_t *input;
    size_t input_len;
    uint8_t *output;
    size_t output_len;               /* >= input_len */
    uint8_t decorrelation_mode;      /* core numbering; forward only */
    bool split_alpha_endpoints;      /* BC3 (BC4 / BC5: split_endpoints, with the switch above on), forward only */
    bool split_colour_endpoints;     /* forward only */
    int32_t status;                  /* out: DXTLT_FF_* */
} DxtltDdsBatchItem;
size_t dxtlt_dds_transform_batch(DxtltDdsBatchItem *items, size_t count, bool inverse);

#ifdef __cplusplus
}
#endif
#endif /* DXTLT_FILE_FORMATS_H */
