/*
 * lh264.h - C ABI of the MI355X-native decode-reconstruct hot path.
 *
 * This is the FINE drop-in boundary of the reference:
 * the reference reconstructs one slice at a time on the CPU through
 *     WelsTargetSliceConstruction(ctx)      codec/decoder/core/src/decode_slice.cpp:110-206
 *       -> WelsTargetMbConstruction         decode_slice.cpp:353-373
 *       -> WelsDeblockingFilterSlice        codec/decoder/core/src/deblocking.cpp:872-934
 *     ExpandReferencingPicture              codec/common/src/expand_pic.cpp:145-174
 * reading the per-macroblock arrays of SDqLayer (codec/decoder/core/inc/dec_frame.h:60-97).
 * Here the same per-macroblock state is handed over as flat records
 * (lh264_mb_t + 384 int16 coefficients per macroblock) and whole batches of
 * frames are reconstructed on the GPU by hand-written gfx950 kernels.
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.
 * Every pointer named *_dev is a device (HBM) address.
 */
#ifndef LH264_H_
#define LH264_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LH264_ABI_VERSION 3

/* ---- macroblock types: the reference's own flag values (codec/common/inc/wels_common_defs.h:264-281) */
#define LH264_MB_I4x4      0x0001
#define LH264_MB_I16x16    0x0002
#define LH264_MB_I8x8      0x0004
#define LH264_MB_P16x16    0x0008
#define LH264_MB_P16x8     0x0010
#define LH264_MB_P8x16     0x0020
#define LH264_MB_P8x8      0x0040
#define LH264_MB_P8x8REF0  0x0080
#define LH264_MB_SKIP      0x0100
#define LH264_MB_IPCM      0x0200
/* ours, not the reference's: a macroblock no slice covered, concealed by the front end (lh264_parser_set_conceal).  The record is
 * LH264_MB_P16x16 | LH264_MB_CONCEAL: one 16x16 prediction with mv[0] and no residual from the picture its slice entry names in
 * ref_slot[0]; it is not filtered, and its neighbours do not filter the edges they share with it */
#define LH264_MB_CONCEAL   0x0400
#define LH264_MB_INTRA     (LH264_MB_I4x4 | LH264_MB_I16x16 | LH264_MB_I8x8 | LH264_MB_IPCM)
#define LH264_MB_INTER     (LH264_MB_P16x16 | LH264_MB_P16x8 | LH264_MB_P8x16 | LH264_MB_P8x8 | LH264_MB_P8x8REF0 | LH264_MB_SKIP)
#define LH264_SUB_8x8 1
#define LH264_SUB_8x4 2
#define LH264_SUB_4x8 4
#define LH264_SUB_4x4 8

/* final (availability-resolved) intra modes, wels_common_defs.h:303-342 */
enum { LH264_I4_V = 0, LH264_I4_H, LH264_I4_DC, LH264_I4_DDL, LH264_I4_DDR, LH264_I4_VR, LH264_I4_HD, LH264_I4_VL,
       LH264_I4_HU, LH264_I4_DC_L, LH264_I4_DC_T, LH264_I4_DC_128, LH264_I4_DDL_TOP, LH264_I4_VL_TOP };
enum { LH264_I16_V = 0, LH264_I16_H, LH264_I16_DC, LH264_I16_P, LH264_I16_DC_L, LH264_I16_DC_T, LH264_I16_DC_128 };
enum { LH264_C_DC = 0, LH264_C_H, LH264_C_V, LH264_C_P, LH264_C_DC_L, LH264_C_DC_T, LH264_C_DC_128 };

#define LH264_MBF_T8x8   0x01   /* transform_size_8x8_flag (pTransformSize8x8Flag) */
#define LH264_MBF_PCM_IN_COEFF 0x02 /* I_PCM: the 384 samples are carried in the coefficient slot (low byte of each int16) */

/* intra_avail bits = pIntraNxNAvailFlag (decode_slice.cpp:567-569, rec_mb.cpp:88-96) */
#define LH264_AVAIL_T  0x1
#define LH264_AVAIL_TL 0x2
#define LH264_AVAIL_L  0x4
#define LH264_AVAIL_TR 0x8

#define LH264_MB_COEFFS 384     /* MB_COEFF_LIST_SIZE, codec/common/inc/wels_const_common.h:55 */
#define LH264_PAD_LUMA   32     /* PADDING_LENGTH, expand_pic.h:49 */
#define LH264_PAD_CHROMA 16
#define LH264_MAX_REFS   16

/*
 * One macroblock, 128 bytes. Field meaning == the SDqLayer array of the same
 * name at index iMbXy (dec_frame.h:60-97) at the moment the reference enters
 * WelsTargetMbConstruction, i.e. after parsing, before any in-place transform.
 */
typedef struct lh264_mb {
  uint16_t mb_type;         /* pMbType                                                   */
  uint8_t  cbp;             /* pCbp: luma bits 0-3, chroma (0..2) << 4                   */
  uint8_t  qp_y;            /* pLumaQp                                                   */
  uint8_t  qp_c[2];         /* pChromaQp[2] (Cb, Cr)                                     */
  uint8_t  flags;           /* LH264_MBF_*                                               */
  uint8_t  intra_avail;     /* pIntraNxNAvailFlag (only I8x8 reads it)                   */
  int8_t   intra_mode[16];  /* pIntra4x4FinalMode[16] (index = raster 4x4 block; I8x8 uses the
                               top-left 4x4 of each 8x8); I16x16: [0] = pIntraPredMode[7] */
  int8_t   chroma_mode;     /* pChromaPredMode                                           */
  uint8_t  reserved0;
  uint16_t slice_id;        /* index into the frame's lh264_slice_t table (pSliceIdc)    */
  uint8_t  sub_type[4];     /* pSubMbType[4]                                             */
  int8_t   ref_idx[4];      /* pRefIndex[LIST_0] of the four 8x8 quadrants               */
  uint8_t  nzc[24];         /* pNzc[24], the reference's raster layout (common_tables.cpp:39-47),
                               as left by the parser (the kernels only test != 0)        */
  int16_t  mv[16][2];       /* pMv[LIST_0][16][2], raster 4x4 blocks, quarter-pel        */
  uint8_t  reserved1[4];
} lh264_mb_t;

/* One slice of a frame (the SSliceHeader fields the hot path reads). */
typedef struct lh264_slice {
  int32_t  first_mb;            /* iFirstMbInSlice                                        */
  int32_t  n_mbs;               /* iTotalMbInCurSlice (consecutive raster MBs; no FMO)    */
  uint8_t  slice_type;          /* 0 = P, 2 = I (EWelsSliceType)                          */
  uint8_t  deblock_idc;         /* uiDisableDeblockingFilterIdc (0,1,2)                   */
  int8_t   alpha_c0_offset;     /* iSliceAlphaC0Offset (already x2, as the reference keeps it) */
  int8_t   beta_offset;         /* iSliceBetaOffset                                       */
  uint8_t  weighted_pred;       /* bUseWeightPredictionFlag                               */
  uint8_t  luma_log2_denom;     /* uiLumaLog2WeightDenom                                  */
  uint8_t  chroma_log2_denom;   /* uiChromaLog2WeightDenom                                */
  uint8_t  n_refs;              /* uiRefCount[0]                                          */
  int16_t  luma_weight[LH264_MAX_REFS];
  int16_t  luma_offset[LH264_MAX_REFS];
  int16_t  chroma_weight[LH264_MAX_REFS][2];
  int16_t  chroma_offset[LH264_MAX_REFS][2];
  int8_t   ref_slot[LH264_MAX_REFS]; /* ref_idx -> index into lh264_frame_job_t.ref (sRefPic.pRefList[LIST_0]); -1: no picture,
                                   the partition then predicts from list entry 0 (rec_mb.cpp:229-233).  RULE: an inter macroblock
                                   whose slice has ref_slot[0] < 0, or whose job has no ref[0], is defined only where ref[0] of the job
                                   is a picture of 128s that nothing writes - the reference reads a null picture there, the oracle
                                   predicts nothing and keeps its fresh picture's 128, the kernel reads job reference 0.  The front
                                   end emits such pictures only in front of a stream's first IDR picture (the IDR was lost);
                                   lh264_decode_batch supplies the 128s, every other caller must not hand such a record to the
                                   device (ReconSession refuses it) */
  uint8_t  luma_dc_weight;      /* Intra-Y 4x4 scaling-list entry [0] (16 = flat): feeds kiQMul of
                                   WelsLumaDcDequantIdct, decode_slice.cpp:272                      */
  uint8_t  reserved[7];
} lh264_slice_t;

/* A picture in HBM: three planes with the reference's padded layout
 * (pic_queue.cpp:62-112): stride = align32(W + 64) luma, half for chroma;
 * plane pointers address pixel (0,0), padding lies at negative offsets. */
typedef struct lh264_pic {
  uint8_t* y_dev;
  uint8_t* u_dev;
  uint8_t* v_dev;
} lh264_pic_t;

/* One frame to reconstruct (== one run of the reference's per-slice loop for every
 * slice NAL of an access unit + ExpandReferencingPicture). */
typedef struct lh264_frame_job {
  const lh264_mb_t*    mbs_dev;     /* mb_w*mb_h records, raster order                    */
  const int16_t*       coeffs_dev;  /* mb_w*mb_h*384, pScaledTCoeff layout*/
  const lh264_slice_t* slices_dev;  /* n_slices entries                                   */
  lh264_pic_t          dst;         /* picture being reconstructed                        */
  lh264_pic_t          ref[LH264_MAX_REFS]; /* reference pictures (deblocked + padded)    */
  int32_t  mb_w, mb_h;
  int32_t  stride_y, stride_c;
  int32_t  n_slices;
  int32_t  flags;                   /* LH264_JOB_* */
} lh264_frame_job_t;

#define LH264_JOB_NO_EXPAND   0x1   /* skip border replication (non-reference picture)    */
#define LH264_JOB_NO_DEBLOCK  0x2   /* debug: stop after reconstruction (pre-deblock planes) */

/* ---- library / device management ----------------------------------------- */
int         lh264_abi_version(void);
/* identifies the build: a hash of the sources the library was compiled from (set by the build recipe, __graft_entry__.build);
 * measurements kept beside the sources (profiles/traffic.json) name the build they were taken on */
const char* lh264_build_id(void);
const char* lh264_last_error(void);
/* number of visible HIP devices (<=0: none; every compute entry point then fails loudly) */
int         lh264_device_count(void);
int         lh264_set_device(int device);

void* lh264_dev_malloc(size_t bytes);
int   lh264_dev_free(void* p_dev);
int   lh264_memcpy_h2d(void* dst_dev, const void* src, size_t bytes, void* hip_stream);
int   lh264_memcpy_d2h(void* dst, const void* src_dev, size_t bytes, void* hip_stream);
int   lh264_dev_memset(void* dst_dev, int value, size_t bytes, void* hip_stream);
int   lh264_stream_sync(void* hip_stream);

/* bytes of one padded picture (all three planes, incl. padding) and the offsets
 * of pixel (0,0) of each plane inside such an allocation. */
size_t lh264_pic_bytes(int mb_w, int mb_h, int* stride_y, int* stride_c,
                       size_t* off_y, size_t* off_u, size_t* off_v);

/* ---- the hot path ---------------------------------------------------------
 * Reconstruct a batch of independent frames: intra/inter prediction + inverse
 * transforms (WelsTargetMbConstruction), in-loop deblocking
 * (WelsDeblockingFilterSlice) and border expansion (ExpandReferencingPicture).
 * jobs_dev: n_jobs descriptors resident in HBM. Frames in one call must not
 * reference each other (a P frame and its reference go in successive calls on
 * the same stream). Asynchronous on hip_stream (NULL = default stream).
 * Returns 0 or a negative LH264_E_* code. */
int lh264_recon_frames(const lh264_frame_job_t* jobs_dev, int n_jobs, int max_mb_w, int max_mb_h,
                       void* hip_stream);

/* Sequential chains: chain c reconstructs jobs_dev[chain_first[c] .. chain_first[c+1]-1]
 * in order inside one workgroup (frames of one stream: P frames may reference
 * earlier jobs of the same chain). chain_first_dev has n_chains+1 entries. */
int lh264_recon_chains(const lh264_frame_job_t* jobs_dev, const int32_t* chain_first_dev, int n_chains,
                       int max_mb_w, int max_mb_h, void* hip_stream);

/* timing helper for bench.py: time `iters` back-to-back invocations of the
 * dominant kernel with hipEvents on the launch stream; returns mean ms per
 * launch (<0 on error). */
double lh264_time_recon_chains(const lh264_frame_job_t* jobs_dev, const int32_t* chain_first_dev, int n_chains,
                               int max_mb_w, int max_mb_h, int iters, void* hip_stream);

/* ---- per-coefficient context-model index -------------------------------------------------
 * For every coefficient symbol of a macroblock the recompressor codes (luma/chroma DC, per-block nonzero count,
 * coefficients in zig-zag order) compute WHICH adaptive prior codes it: the flat index into the reference's
 * tables lumaDCIntPriors / chromaDCIntPriors / nonzerosPriors[8x8] / acPriors[8x8] (macroblock_model.h:45-53),
 * i.e. what getLumaDCIntPrior, getChromaDCIntPrior, getNonzerosPrior4x4/8x8 and getACPrior4x4/8x8
 * (macroblock_model.cpp:466-594) return, driven like encode4x4 (decode_slice.cpp:2059-2094, 2393-2434).
 * The adaptive update and the arithmetic coder (rows a9/a10) consume these symbols on the host side. */
typedef struct lh264_ctx_sym {
  uint32_t prior;     /* flat index into the table selected by `kind`                                  */
  int16_t  value;     /* the integer that is coded with that prior                                     */
  uint8_t  kind;      /* LH264_SYM_*                                                                   */
  uint8_t  pad;       /* the tag the symbol's decisions are billed to (billing.h:6-55), part of the symbol: the coder takes a nonzero
                         pad as it stands.  lh264_ctx_index_chains writes 17 for LUMA_DC, 18 for CHROMA_DC; for NZ4/NZ8 29 in a chroma
                         block and 19 in a luma block; for AC4/AC8 29 in a chroma block, 19 for the first coefficient symbol of a luma
                         block whose macroblock is not Intra16x16, and 24 for every other luma one.  0 = not given: the coder then
                         takes the tag of a coefficient symbol out of `prior`                                          */
} lh264_ctx_sym_t;
enum { LH264_SYM_LUMA_DC = 0, LH264_SYM_CHROMA_DC = 1, LH264_SYM_NZ4 = 2, LH264_SYM_AC4 = 3, LH264_SYM_NZ8 = 4, LH264_SYM_AC8 = 5,
       /* the non-coefficient syntax symbols (row a10), produced by the host front end; for these `prior` is
        * LH264_PRIOR(table, index) and `pad` the tag the decisions go to (billing.h:6-55) */
       LH264_SYM_TREE = 6,    /* value coded MSB first through a binary tree of priors (Branch<n>, compression_stream.h:117-166) */
       LH264_SYM_POW2 = 7,    /* emitBitsZeroToPow2Inclusive<n> (:455-463): flag "differs from the preferred value" + tree      */
       LH264_SYM_BIT = 8,     /* one decision with its own prior                                                             */
       LH264_SYM_RAW = 9,     /* `prior` raw bits of `value`, MSB first, through the shared adaptive TEST_PROB (:441-448)      */
       LH264_SYM_MVD = 10,    /* emitUEGkInt with MotionVectorDifferencePrior = UEGkIntPrior<9,4,3,4,3> (:575-591)            */
       LH264_SYM_SPLICE = 15  /* marker in a host list: the macroblock's coefficient symbols (rows a8) go here             */ };
#define LH264_CTX_MAX_SYMS 432   /* 16 + 8 + 24 + 384 symbols per macroblock at most */
/* prior tables of the reference's MacroblockModel (macroblock_model.h:36-136) */
enum { LH264_TB_MBTYPE = 0, LH264_TB_MVD, LH264_TB_MODE8, LH264_TB_LDC, LH264_TB_CDC, LH264_TB_NZ4, LH264_TB_NZ8, LH264_TB_AC4, LH264_TB_AC8,
       LH264_TB_SKIPRUN, LH264_TB_QPL, LH264_TB_SUBMB, LH264_TB_NUMREF, LH264_TB_CBPC, LH264_TB_CBPL, LH264_TB_STOP, LH264_TB_T8,
       LH264_TB_PREDMODE, LH264_TB_COUNT };
#define LH264_PRIOR(table, index) (((uint32_t)(table) << 27) | (uint32_t)(index))
#define LH264_MAX_SYN_SYMS 96    /* non-coefficient symbols of one macroblock at most (incl. the splice marker and a slice's pad bits) */

/* One frame of context-index work.  `levels` = the raw (not dequantised) coefficient levels in the
 * pScaledTCoeffQuant layout (what the reference copies into DecodedMacroblock::odata, decode_slice.cpp:69-79).
 * nnz images: 24 bytes per macroblock = per-4x4 nonzero counts (DecodedMacroblock::countSubblockNonzeros) of the
 * reference's FreqImage entry of that position: a skipped macroblock inherits the PAST entry
 * (decode_slice.cpp:3104-3108).  The host decides which earlier frame is PAST (frame_num flips, resolution
 * changes: decoded_macroblock.h:119-123, decode_slice.cpp:3032-3046) by pointing nnz_past_dev at its image.
 * A macroblock no slice covers (mb_type 0: a lost slice) is not written by the reference at all: its entry stays what the picture that
 * last occupied the SAME FreqImage buffer left there (KEEP).  The struct has no field for that image: lh264_ctx_index_chains gives such
 * a macroblock the PAST entry, lh264_ctx_index_chains_keep takes the KEEP images beside the jobs. */
typedef struct lh264_ctx_job {
  const lh264_mb_t*    mbs_dev;       /* mb_w*mb_h records                                       */
  const int16_t*       levels_dev;    /* mb_w*mb_h*384                                           */
  const lh264_slice_t* slices_dev;
  const uint8_t*       nnz_past_dev;  /* mb_w*mb_h*24 or NULL (no PAST); KEEP: lh264_ctx_index_chains_keep */
  uint8_t*             nnz_cur_dev;   /* mb_w*mb_h*24, written by pass 1, read by pass 2 and later frames */
  lh264_ctx_sym_t*     syms_dev;      /* the symbols, emission order.  FIXED layout (sym_off_dev == NULL): mb_w*mb_h*LH264_CTX_MAX_SYMS slots,
                                         macroblock k at k*LH264_CTX_MAX_SYMS, first n_syms[k] valid.  COMPACT layout: see below       */
  uint16_t*            n_syms_dev;    /* mb_w*mb_h                                               */
  int32_t  mb_w, mb_h;
  /* COMPACT layout (ABI 3; sym_off_dev != NULL): the jobs of a call share ONE pool of symbols - syms_dev is the pool's first symbol in
   * every job, syms_cap its size in symbols -, macroblock k of this picture lies at syms_dev[*sym_base_dev + sym_off_dev[k]].  Both
   * are WRITTEN by the call (a count pass over the levels: 8 bytes per coded symbol instead of 3,456 bytes per macroblock).  The
   * offsets are DENSE: sym_off_dev[k] is the sum of n_syms of the picture's macroblocks before k, *sym_base_dev the sum over the
   * compact jobs before this one (a job in the fixed layout counts as 0); there is no padding between runs.  The pool is sized from
   * lh264_ctx_count_chains.  Where it is too small, nothing at or beyond syms_cap symbols is written: a macroblock whose run ends at or
   * before syms_cap is written whole with its n_syms, every other macroblock writes nothing and reads n_syms 0; sym_off, *sym_base and
   * the *total_dev of the count call still tell the need. */
  uint32_t*            sym_off_dev;   /* mb_w*mb_h offsets (symbols) behind the picture's first symbol              */
  uint64_t*            sym_base_dev;  /* this picture's first symbol in the pool (one word per job)                 */
  uint64_t             syms_cap;      /* symbols there is room for at syms_dev                                      */
} lh264_ctx_job_t;

/* chains as in lh264_recon_chains (frames of one stream in order: the nnz image of a frame may be the PAST of a
 * later one).  Pass 1 (nnz images) runs one workgroup per chain, pass 2 (symbols) one wave per macroblock. */
int lh264_ctx_index_chains (const lh264_ctx_job_t* jobs_dev, const int32_t* chain_first_dev, int n_chains,
                            int n_jobs, int max_mbs_per_frame, void* hip_stream);
/* The same for pictures with lost slices.  A macroblock whose record has mb_type 0 (no slice covers it) has no symbols; the two
 * calls above give it the PAST entry, like a skipped one.  The reference's FreqImage does not: a cell that no slice writes keeps what
 * the last picture in the SAME buffer left there.  keep_dev: a device array of n_jobs pointers, keep_dev[j] = the nnz image (mb_w*mb_h*24
 * bytes) of the picture that last occupied the buffer picture j goes to - the picture before when frame_num did not change, else the
 * one two flips back -, an earlier job of the same chain or a buffer the caller carried; NULL = no KEEP (the stream's first pictures,
 * after a change of size): zeros.  Macroblocks of type 0 take their entry from there, skipped ones from PAST as ever.  keep_dev ==
 * NULL: exactly the calls above. */
int lh264_ctx_index_chains_keep (const lh264_ctx_job_t* jobs_dev, const uint8_t* const* keep_dev, const int32_t* chain_first_dev, int n_chains,
                                 int n_jobs, int max_mbs_per_frame, void* hip_stream);
int lh264_ctx_count_chains_keep (const lh264_ctx_job_t* jobs_dev, const uint8_t* const* keep_dev, const int32_t* chain_first_dev, int n_chains,
                                 int n_jobs, int max_mbs_per_frame, unsigned long long* total_dev, void* hip_stream);
/* COMPACT layout, first half: pass 1 and the count alone - fills n_syms_dev, sym_off_dev and *sym_base_dev of every job and
 * *total_dev = the symbols of all jobs (what the pool must hold).  lh264_ctx_index_chains repeats this on its own: the call exists so
 * that the caller can size the pool. */
int lh264_ctx_count_chains (const lh264_ctx_job_t* jobs_dev, const int32_t* chain_first_dev, int n_chains,
                            int n_jobs, int max_mbs_per_frame, unsigned long long* total_dev, void* hip_stream);

/* ---- rows a9 + a10 + f4: the adaptive binary arithmetic coder, on the device -----------------------------------
 * Consumes, per macroblock in coding order, the host list of syntax symbols (with the SPLICE marker where the
 * coefficient symbols of lh264_ctx_index_chains go) and produces the byte string of every tagged stream exactly as
 * the reference's compressor writes it to <out>.pip.<tag> (ArithmeticCodedOutput / vpx_writer,
 * compression_stream.h:353-487, bitwriter.h:35-105; DynProb :87-115; emitInt / emitUEGkInt :523-591).
 * The stream's symbols are binarised in parallel (one wave per macroblock); the adaptive probabilities are resolved by one
 * workgroup per stream, 64 decisions per wave step; one lane per (stream, tag) runs the bool coder.  The adaptive priors live in
 * the LDS of the stream's workgroup; what does not fit is spilled to a per-stream open-addressing table in HBM (hash_cells_dev:
 * hash_cap x 64 bytes = 8 x hash_cap entries of one DynProb each, zero-filled by the caller; a stream of N macroblocks touches
 * roughly 2 N DynProbs, QCIF ... 1080p content measured). */
#define LH264_N_TAG_SLOTS 40
typedef struct lh264_code_job {
  const lh264_ctx_sym_t* syn_syms_dev;   /* host symbols of the picture, macroblock after macroblock        */
  const uint32_t*        syn_off_dev;    /* n_mbs + 1 offsets into syn_syms_dev                             */
  const lh264_ctx_sym_t* ctx_syms_dev;   /* lh264_ctx_job_t.syms_dev: n_mbs * LH264_CTX_MAX_SYMS, or the pool    */
  const uint16_t*        ctx_n_syms_dev; /* n_mbs                                                           */
  int32_t n_mbs, reserved;
  const uint32_t*        ctx_sym_off_dev;  /* lh264_ctx_job_t.sym_off_dev (NULL: the fixed layout)          */
  const uint64_t*        ctx_sym_base_dev; /* lh264_ctx_job_t.sym_base_dev                                  */
} lh264_code_job_t;
typedef struct lh264_code_stream {
  uint32_t* hash_keys_dev;     /* not used (ABI 1 kept the keys of the table here)                          */
  uint32_t* hash_cells_dev;    /* hash_cap * 16 words, zero-filled: the spill table of the adaptive priors  */
  uint8_t*  out_dev;           /* LH264_N_TAG_SLOTS * out_cap bytes: slot t at t * out_cap                  */
  uint32_t* out_len_dev;       /* LH264_N_TAG_SLOTS lengths (0: tag never used); [LH264_N_TAG_SLOTS] = status (0 ok) */
  uint32_t  hash_cap;          /* power of two, at most 1 << 20                                             */
  uint32_t  out_cap;
} lh264_code_stream_t;
/* tag id (billing.h) <-> slot: slot = tag for tags < 34, slot 34 = tag 69 (pad bits).
 * chain_first_dev: n_chains + 1 entries (stream c codes jobs_dev[chain_first[c] .. chain_first[c+1]-1] in order); n_jobs = all
 * pictures, total_mbs = the sum of their n_mbs, max_mbs_per_frame = the largest n_mbs.  The call sizes its work memory (kept
 * between calls, per device) from a count pass, so it synchronises hip_stream once in the middle; the tagged streams are complete
 * when hip_stream has drained.  out_len_dev[LH264_N_TAG_SLOTS] != 0 reports (bits): 1 prior table full or hash_cap invalid (not a power of
 * two, zero, above 1 << 20, or - with the per-partition tables of large streams - below 8 entries x the partition count), 4 output
 * overflow (the lengths then say how much room is needed), 8 counter overflow (2^32 decisions or 2^27 list entries in one stream, or
 * total_mbs smaller than the pictures' macroblock counts), 16 internal (a hand-off between the waves of a stream timed out / the range
 * walk lost its state: the result is wrong; never seen outside broken development builds).  Any non-zero status: the stream's tagged
 * bytes must not be used.
 * Coder calls share one set of work memory per device: calls on different HIP streams are ordered on the device by an event (a later call
 * waits for the earlier one's kernels), calls on one stream by the stream. */
int lh264_code_chains (const lh264_code_job_t* jobs_dev, const int32_t* chain_first_dev, const lh264_code_stream_t* streams_dev,
                       int n_chains, int n_jobs, long long total_mbs, int max_mbs_per_frame, void* hip_stream);
/* The same in two calls, for a caller that wants to put other work between the halves (the second half - the adaptive probabilities
 * and the bool coders - is two serial chains whose waves mostly wait: it runs well beside a kernel that is bound by arithmetic,
 * e.g. lh264_recon_chains on another stream; the first half - binarisation - does not).  lh264_code_binarise_chains counts and
 * writes the decision words (it is the half that synchronises hip_stream once); lh264_code_finish_chains must follow on the same
 * device with the same streams_dev and n_chains, before any other coder call there. */
int lh264_code_binarise_chains (const lh264_code_job_t* jobs_dev, const int32_t* chain_first_dev, const lh264_code_stream_t* streams_dev,
                                int n_chains, int n_jobs, long long total_mbs, int max_mbs_per_frame, void* hip_stream);
int lh264_code_finish_chains (const lh264_code_stream_t* streams_dev, int n_chains, void* hip_stream);
/* ---- resumable calls: a stream of any length, coded in SEGMENTS of whole pictures, one call after another ----------------------
 * lh264_code_chains_resume codes the pictures of chain c as the NEXT segment of stream c; what the stream's coders have to remember
 * between two calls lies in carry_dev[c], an opaque block of lh264_code_carry_bytes (hash_cap) bytes of device memory that the caller
 * zero-fills before the stream's first segment and keeps until its last: every adaptive probability the stream has touched with its
 * exact counters (the block holds the stream's spill table; streams_dev[c].hash_cells_dev is not used, hash_cap must be the same in
 * every segment), and per tag whether the stream exists, the coder's range, the bits shifted out and the decisions coded so far.
 * flags_dev[c]: LH264_CODE_SEG_FIRST - the stream starts here (the block's header is initialised by the call) -, LH264_CODE_SEG_LAST -
 * the bool coders are stopped (the 32 padding decisions and the trailing-zero rule happen here and only here).  A call may mix streams
 * in their first, a middle and their last segment; FIRST | LAST gives what lh264_code_chains gives.  out_dev / out_cap are the same
 * buffer in every segment and are appended to: after the LAST segment out_len_dev holds the lengths as lh264_code_chains leaves them;
 * after any other it holds, per tag, how many bytes are FINAL (a carry out of a later segment's bytes can still run back through a
 * run of 0xff bytes and into the byte in front of it: the call applies it; the two bytes behind the written ones are work space).
 * The bytes do not depend on where the cuts fall.  Status bits as in lh264_code_chains, per segment and sticky: a stream that failed
 * fails in every later segment - except status 8, which the count pass gives before anything is coded: the carry stands as it was and
 * the caller sends a shorter segment.  The 2^32 / 2^27 limits are limits of ONE segment; both count the decisions of ALL tag lists of
 * the stream together (a decision word addresses the stream's lists as one array), not those of one tag.  Always the wave-per-partition form; calls on one
 * stream's carry must be ordered (one HIP stream, or the caller's events).  device memory only, all pointers. */
#define LH264_CODE_SEG_FIRST 1u
#define LH264_CODE_SEG_LAST  2u
size_t lh264_code_carry_bytes (uint32_t hash_cap);
int lh264_code_chains_resume (const lh264_code_job_t* jobs_dev, const int32_t* chain_first_dev, const lh264_code_stream_t* streams_dev,
                              void* const* carry_dev, const uint32_t* flags_dev,
                              int n_chains, int n_jobs, long long total_mbs, int max_mbs_per_frame, void* hip_stream);
/* decisions coded into every tag slot's list of the stream so far (LH264_N_TAG_SLOTS x uint64, host memory), summed over its segments;
 * synchronises hip_stream */
int lh264_code_carry_decisions (const void* carry_dev, uint64_t* decisions_out, void* hip_stream);
/* decisions per tag slot of chains first_chain .. first_chain + n_chains - 1 of the last coder call on the current device (n_chains x
 * LH264_N_TAG_SLOTS values, host memory; of a resumable call: of that segment).  Synchronises the device.  A stream whose status is not
 * 0 reads 0 for the tags its range stage dropped.  "The last call" is per device, not per caller: a thread that wants its own call's
 * counts must keep other coder calls off the device between the call and this read (lh264_compress_batch does, for its own groups, by
 * its per-device lock; direct coder calls from other threads are the caller's to order). */
int lh264_code_last_decisions (int first_chain, int n_chains, uint64_t* decisions_out);
/* sizes of the last lh264_code_chains call on the current device: 64-bit decision words written and read between its stages (one
 * per binary decision, each stream's count rounded up to 64) and 16-bit tag-list entries (one per decision, each tag's list padded
 * to 8): what the coder's memory traffic is computed from (bench.py). */
int lh264_code_last_totals (unsigned long long* decision_words, unsigned long long* list_entries);

/* ---- host front end: Annex-B bitstream -> macroblock records ------------------------------
 * Replaces, for the records the hot path needs, the reference's WelsDecodeBs / ParseNonVclNal / slice-header parse /
 * CAVLC macroblock parse (decoder.cpp:658-860, au_parser.cpp, decode_slice.cpp:3173-3984, parse_mb_syn_cavlc.cpp).
 * Pure host code.  Pictures come out in decode order (I and P slices only, as in the reference). */
typedef struct lh264_parser lh264_parser_t;
typedef struct lh264_frame_info {
  int32_t id, mb_w, mb_h, n_slices, n_refs, frame_num;
  int32_t crop_x, crop_y, crop_w, crop_h;      /* cropped output window in luma samples (SBufferInfo iWidth/iHeight) */
  int32_t is_ref, idr;
  int32_t ref_ids[LH264_MAX_REFS];             /* picture ids behind this picture's job ref slots */
} lh264_frame_info_t;
lh264_parser_t* lh264_parser_create (void);
void  lh264_parser_destroy (lh264_parser_t* p);
/* feed Annex-B bytes ending on a NAL boundary; flush != 0 completes the picture in progress. <0 on a parse error
 * (lh264_parser_error gives the text; pictures parsed so far stay available) */
int   lh264_parser_feed (lh264_parser_t* p, const uint8_t* data, size_t len, int flush);
/* a whole Annex-B file, cut into chunks and fed the way the reference's console application does (h264dec.cpp:246-272,
 * one ISVCDecoder::DecodeFrameNoDelay per start-code-delimited chunk), flush included.  Besides the pictures this builds
 * the recompressor's default stream (stream id 0x7fffffff, the ".pip" file itself: the input minus its slice data,
 * decoder.cpp:658-860, au_parser.cpp:143,588, decode_slice.cpp:2974-2980), returned by lh264_parser_main_stream */
int   lh264_parser_feed_file (lh264_parser_t* p, const uint8_t* data, size_t len);
/* the same file in pieces, for streams of any length: lh264_parser_begin_file, then lh264_parser_feed_file_some until it returns 1 (the
 * file is finished: last picture completed, default stream whole; 0: there is more; < 0: bad argument).  A call returns as soon as the
 * parser holds MORE than want_mbs macroblocks in completed pictures; the caller takes pictures from the front and releases them with
 * lh264_parser_drop_frames (p, n) - the pictures that remain are renumbered from 0, their records are what the whole parse gives -, so
 * the parser's memory follows want_mbs and not the file's length.  data must stay valid until the file is finished; a parse error
 * is reported by lh264_parser_error as ever. */
int   lh264_parser_begin_file (lh264_parser_t* p, const uint8_t* data, size_t len);
int   lh264_parser_feed_file_some (lh264_parser_t* p, uint64_t want_mbs);
int   lh264_parser_drop_frames (lh264_parser_t* p, int n);
const uint8_t* lh264_parser_main_stream (const lh264_parser_t* p, size_t* len);
/* the samples of the stream's I_PCM macroblocks (384 bytes each, decoding order): stream LH264_TAG_PCM of the container, see
 * lh264_pip_restore */
const uint8_t* lh264_parser_pcm_samples (const lh264_parser_t* p, size_t* len);
int   lh264_parser_frame_count (const lh264_parser_t* p);
int   lh264_parser_frame_info (const lh264_parser_t* p, int idx, lh264_frame_info_t* out);
const lh264_mb_t*    lh264_parser_frame_mbs (const lh264_parser_t* p, int idx);
const int16_t*       lh264_parser_frame_coeffs (const lh264_parser_t* p, int idx);
const int16_t*       lh264_parser_frame_levels (const lh264_parser_t* p, int idx);
/* sparse coefficients (set before the first byte is fed): lh264_parser_frame_coeffs is NULL and the picture's nonzero dequantised
 * coefficients - of an I_PCM macroblock its nonzero samples - come as a list, ascending:
 * (picture-relative macroblock * 384 + position) << 16 | (uint16_t) value.  What lh264_decode_batch uploads instead of 768 bytes per
 * macroblock; a kernel scatters it into planes cleared on the device */
/* concealment of lost slices (set before the first byte is fed; LH264_CONCEAL_*, 0 = off, the default): a completed picture with
 * macroblocks no slice covers gets their records filled - mb_type LH264_MB_P16x16 | LH264_MB_CONCEAL, the final vector in mv[], a slice
 * entry appended to the picture's table whose ref_slot[0] names the source picture (a slot past n_refs: the picture of 128s) - the way
 * the reference's decoder conceals them (error_concealment.cpp); lh264_parser_frame_covered still says which they were.  For the decode
 * direction only.  LH264_E_ARG: a method that is not provided.  lh264_parser_frame_conceal: out[0] the number of concealed macroblocks,
 * [1] the source picture's id or -1, [2] 1 when the picture is withheld from the output (the FREEZE methods), [3..4] the mean vector
 * of the received inter partitions with ref_idx 0, [5..6] the vector before the per-macroblock clamp, [7] this picture's POC as the
 * reference counts it (pic_order_cnt_lsb), [8] list entry 0's, [9] the source's, [10] 0 = copy, 1 = the mean, 2 = the mean scaled by
 * the POC distances, [11] the picture's POC once it is done (what a later picture's scaling reads: 0 behind an mmco 5); set for
 * every picture, concealed or not */
#define LH264_CONCEAL_OFF                            0
#define LH264_CONCEAL_SLICE_COPY                     2   /* the values of the reference's ERROR_CON_IDC (codec_app_def.h) */
#define LH264_CONCEAL_SLICE_COPY_CROSS_IDR           4
#define LH264_CONCEAL_SLICE_COPY_CROSS_IDR_FREEZE    5   /* ..._FREEZE_RES_CHANGE */
#define LH264_CONCEAL_SLICE_MV_COPY_CROSS_IDR        6
#define LH264_CONCEAL_SLICE_MV_COPY_CROSS_IDR_FREEZE 7   /* ..._FREEZE_RES_CHANGE */
int                  lh264_parser_set_conceal (lh264_parser_t* p, int method);
int                  lh264_parser_frame_conceal (const lh264_parser_t* p, int idx, int32_t out[12]);
int                  lh264_parser_set_sparse_coeffs (lh264_parser_t* p, int on);
/* deferred slice data (set before the first byte is fed; off by default, and then nothing changes): the header of a CAVLC slice is walked -
 * picture boundaries, reference lists, marking, the entry in the slice table - and its macroblock layer is not parsed; the slice is kept
 * with its picture (payload, where slice_data() begins, a copy of its header and parameter sets).  Records, coefficients, `covered`,
 * n_mbs and the slice syntax of such a slice stay empty until lh264_parser_parse_deferred runs the host macroblock layer over it - to be
 * called for the slices 0 .. lh264_parser_frame_deferred - 1 of a completed picture in order; 1: parsed, 0: the slice failed (then
 * lh264_parser_error / _error_pictures / _file_status say what the undeferred parser says); out (may be NULL): the slice's index in
 * the picture's slice table and the bit position at which the macroblock layer stopped.  CABAC slices are parsed on the spot, unless
 * lh264_parser_set_defer_cabac is on as well: then they are deferred like the CAVLC ones (lh264_parser_frame_deferred counts both,
 * lh264_parser_frame_deferred_cabac tells 1 for a CABAC slice, 0 for a CAVLC one, LH264_E_ARG for no slice), lh264_parser_parse_deferred
 * runs the host's CABAC layer over them and the position it reports is the arithmetic decoder's: the number of the next bit it would
 * take in.  lh264_parser_set_defer_cabac on its own does nothing; lh264_parser_set_defer_slice_data keeps its meaning whatever its value.
 * For the decode direction: symbol lists, I_PCM samples and concealment are not kept up for deferred pictures.
 * lh264_parser_error_pictures: how many pictures were complete when lh264_parser_error was raised; lh264_parser_file_status: what
 * lh264_parser_feed_file returned, or would return now */
int                  lh264_parser_set_defer_slice_data (lh264_parser_t* p, int on);
int                  lh264_parser_set_defer_cabac (lh264_parser_t* p, int on);
int                  lh264_parser_frame_deferred (const lh264_parser_t* p, int idx);
int                  lh264_parser_frame_deferred_cabac (const lh264_parser_t* p, int idx, int slice);
int                  lh264_parser_parse_deferred (lh264_parser_t* p, int idx, int slice, int32_t out[2]);
long long            lh264_parser_error_pictures (const lh264_parser_t* p);
int                  lh264_parser_file_status (const lh264_parser_t* p);
const uint64_t*      lh264_parser_frame_sparse_coeffs (const lh264_parser_t* p, int idx, size_t* count);
const lh264_slice_t* lh264_parser_frame_slices (const lh264_parser_t* p, int idx);
const uint8_t*       lh264_parser_frame_covered (const lh264_parser_t* p, int idx);
/* row a10: the macroblock syntax the recompressor codes beyond lh264_mb_t (the reference's DecodedMacroblock fields,
 * decoded_macroblock.h:12-34): one packed 116-byte lh264_mbsyn_t per macroblock, and per slice 4 x int32
 * {alignment bit count after the stop bit, their value, PPS transform_8x8_mode_flag,
 * flags: bit 0 entropy_coding_mode_flag, bit 1 constrained_intra_pred_flag} */
typedef struct lh264_mbsyn {
  uint8_t  have, slice_type, t8, cbp_c, cbp_l, chroma_mode, luma16_mode, luma_qp;
  uint8_t  mb_type[4], num_ref_idx_l0[4], skip_run[4];   /* little-endian u32 / u32 / i32 (the struct is byte-packed) */
  int8_t   ref_idx[4];
  uint8_t  sub_type[4];
  int8_t   pred_mode[16];
  uint8_t  mvd[64];                                      /* int16 [16][2], little-endian */
  uint8_t  delta_qp[4], last_mb_qp[4];                   /* i32 */
} lh264_mbsyn_t;
const lh264_mbsyn_t* lh264_parser_frame_syntax (const lh264_parser_t* p, int idx);
const int32_t*       lh264_parser_frame_slice_syntax (const lh264_parser_t* p, int idx);
/* the row-a10 symbols of the picture (LH264_SYM_TREE .. LH264_SYM_SPLICE) and mb_w*mb_h + 1 offsets into them */
const lh264_ctx_sym_t* lh264_parser_frame_syn_symbols (const lh264_parser_t* p, int idx, int* count);
const uint32_t*      lh264_parser_frame_syn_offsets (const lh264_parser_t* p, int idx);
const char*          lh264_parser_error (const lh264_parser_t* p);
/* "" or why lh264_compress_batch refuses the stream although it parses: the first syntax value met so far that the container's prior
 * tables cannot carry ("mb_skip_run 687 is outside the container's range 0..511"); such a stream is stored verbatim */
const char*          lh264_parser_out_of_range (const lh264_parser_t* p);
/* LH264_COMPRESS_TOLERANT for a parser: to be called before the first byte is fed (LH264_E_ARG afterwards).  The default stream then
 * keeps the payload of every NAL unit that is not handed to the model as a slice. */
int                  lh264_parser_set_tolerant (lh264_parser_t* p, int on);
/* "" or a text naming the first NAL unit met so far whose bytes the default stream does not keep with the flag off (its place in the
 * file, counted from 0, its type and the byte offset of its header byte): the stream needs LH264_COMPRESS_TOLERANT to restore.  The
 * same text whether the flag is on or off.  No device is needed. */
const char*          lh264_parser_not_kept (const lh264_parser_t* p);
/* "" or a text naming the first NAL unit that the default stream cannot carry even with the flag (see LH264_COMPRESS_TOLERANT): why
 * lh264_compress_batch_opts refuses the stream under the flag */
const char*          lh264_parser_not_carried (const lh264_parser_t* p);
/* what carries those values all the same: the escape stream of the pictures parsed so far (stream LH264_TAG_ESC of the container, see
 * lh264_pip_restore for the format), runs still open closed; *len = 0 when no value was out of range, and also when one was that the
 * escape stream cannot carry (17 or more active references, a value of another table): such a stream stays refused.  A finished copy at any time -
 * lh264_parser_drop_frames does not touch it -, valid until the next call for this parser */
const uint8_t*       lh264_parser_escapes (const lh264_parser_t* p, size_t* len);

/* ---- restore direction, host side ------------------------------------------------------------
 * The inverse of compress: the default stream (".pip") plus the tagged arithmetic-coded streams (".pip.<tag>") -> the
 * original Annex-B bytes (what `h264dec in.pip out.264` does in the reference: decode_slice.cpp:2476-2936, decoder.cpp:658-860).
 * tags[t] / tag_len[t] are indexed by tag id (billing.h:6-55), n_tags >= 70 to include the pad-bit tag 69; NULL = no such
 * stream.  *out_len receives the restored size; LH264_E_ARG when out_cap is too small (then *out_len = the size needed).
 * I_PCM macroblocks: the reference's representation does not carry their samples (its own restore aborts on them); ours adds one
 * stream, tags[LH264_TAG_PCM] = the 384 samples of every I_PCM macroblock in decoding order, stored as they are.  With it streams
 * with I_PCM macroblocks restore (CAVLC: 7.3.5; CABAC: the engine is flushed before the samples and restarted behind them,
 * 9.3.1.2); without it the call gives LH264_E_UNSUPPORTED (lh264_restore_error: the text).
 * Values above a prior table's tree: an mb_skip_run above 511 (SKIPRUN is a 9-bit tree) and num_ref_idx_l0_active 16 (NUMREF is a
 * 4-bit tree) are coded modulo the tree, as the reference codes them; tags[LH264_TAG_ESC] carries what the tree drops.  It is a
 * sequence of entries of four unsigned LEB128 varints {table, gap, high, repeat}: table is LH264_TB_SKIPRUN or LH264_TB_NUMREF; gap
 * counts the tree symbols of that table, in coding order, between the end of the table's previous entry (or the stream's start) and
 * the entry's first symbol (every SKIPRUN / NUMREF symbol counts: CABAC slices and I slices have one SKIPRUN per macroblock); high >= 1
 * is the value >> the tree's bits; repeat >= 1 is how many consecutive symbols of the table carry this high.  Entries of one table
 * are in order, those of the two tables interleave as their runs close; the runs open at the end are closed SKIPRUN first.  A stream
 * without such a value has no such tag.  The tag is honoured whenever it is present, by this call and by the device restore alike; a
 * malformed one (unknown table, high or repeat 0, a truncated varint or one wider than 64 bits, a restored num_ref_idx above 16, entries
 * left over at the end of the default stream) is LH264_E_UNSUPPORTED with a text, never other bytes. */
#define LH264_TAG_PCM 70
#define LH264_TAG_ESC 71
int lh264_pip_restore (const uint8_t* main_stream, size_t main_len, const uint8_t* const* tags, const size_t* tag_len, int n_tags,
                       uint8_t* out, size_t out_cap, size_t* out_len);
const char* lh264_restore_error (void);       /* message of the calling thread's last failed lh264_pip_restore */

/* ---- single-file container: the default stream and the tagged streams in one file, or - flag VERBATIM - the
 * input itself for streams the round trip cannot carry (damaged streams, syntax the front end does not parse) or does not shrink, so that
 * every input restores.  Layout: "LHPIP1\0\0", u32 flags, u32 n, n x {u32 stream id (0x7fffffff = default stream, else the
 * tag id), u32 length}, the payloads in that order; little endian.  The reference has no counterpart (it writes one file per
 * stream, h264dec.cpp:79-104, and aborts on what it cannot restore). */
#define LH264_PIP_VERBATIM 1u
size_t lh264_pip_pack_bound (size_t main_len, const size_t* tag_len, int n_tags);
int lh264_pip_pack (const uint8_t* main_stream, size_t main_len, const uint8_t* const* tags, const size_t* tag_len, int n_tags,
                    uint32_t flags, uint8_t* out, size_t out_cap, size_t* out_len);
/* restore from a container: lh264_pip_restore on its streams, or a copy of the payload when it is VERBATIM */
int lh264_pip_restore_file (const uint8_t* file, size_t len, uint8_t* out, size_t out_cap, size_t* out_len);

/* ---- the whole compress direction behind one call (host orchestration in C++; what the Python sessions of this repository do)
 * n independent Annex-B files -> per stream the default stream and the tagged streams, exactly the files the reference's console
 * application writes (h264dec.cpp:79-121): host front end on `threads` host threads (0 = all), one lh264_ctx_index_chains and
 * one lh264_code_chains launch per sub-batch on the current device, results copied back.  Every out[i] is a handle to free;
 * lh264_compressed_status tells whether stream i compressed (LH264_OK) or why not (LH264_E_UNSUPPORTED: syntax the front end
 * does not parse; LH264_E_HIP ...), lh264_compressed_error gives the text. */
typedef struct lh264_compressed lh264_compressed_t;
int lh264_compress_batch (const uint8_t* const* data, const size_t* len, int n, int threads, lh264_compressed_t** out);
/* the same over several devices of one node: contiguous shares of about equal input size, one host thread per device driving
 * lh264_compress_batch there (the streams are independent: nothing is exchanged between devices) */
int lh264_compress_batch_devices (const uint8_t* const* data, const size_t* len, int n, int threads, const int* devices, int n_devices,
                                  lh264_compressed_t** out);
/* the same with options.  segment_mbs: a stream of more macroblocks than this is cut at picture boundaries into segments of at most
 * that many (one picture at least); its segments go through successive groups, in order, coded by lh264_code_chains_resume with the
 * stream's state carried in device memory, and its pictures are parsed a segment ahead and released segment by segment, so that host
 * and device memory follow the segment's size and not the stream's length (the final bytes of every tag go to the host segment by
 * segment; what grows with the stream is the result itself).  0 = the default, the group budget (1,300,000 macroblocks): no stream that fits a group is cut.  A segment that is
 * over one of the coder's per-call limits (status 8: 2^27 decisions in all tags of the stream together) is sent again with half the
 * pictures - a whole stream that is over them becomes a long one -, and segments are cut by an estimate of their decisions first, so
 * that this is rare; status 8 reaches the caller only for a single picture.  A long stream that fails in any segment has the error as
 * its result and no tags.  The bytes do not depend on where the cuts fall.  A struct_bytes this library does not know: LH264_E_ARG.
 * `reserved` is the flags word (the field keeps the name it was declared with; 0 as callers have always passed it = no flag):
 * LH264_COMPRESS_ESCAPES - a stream that lh264_parser_out_of_range names, and nothing else stands against, is compressed and
 * gets the escape stream lh264_parser_escapes as tag LH264_TAG_ESC (every other tag and the default stream are what they are without
 * the flag's guard: the reference's own files); without the flag it is refused as ever.  Streams inside the range are not touched by
 * the flag.  An unknown flag: LH264_E_ARG.
 * LH264_COMPRESS_TOLERANT - streams with NAL units the format drops and pictures with lost slices are compressed.
 *  (a) KEPT: with the flag the default stream keeps the payload (the unescaped bytes behind the header byte, without the trailing zero
 *  bytes) of EVERY NAL unit that is not handed to the model as a slice - types 2-4 and 9-31, and a PPS in front of the first SPS -, as
 *  it always did for types 6, 7 and 8; without the flag it keeps the header byte of those and drops the rest, as the reference does
 *  (lh264_parser_not_kept tells beforehand), and the call returns LH264_OK for a stream that does not restore.  The restorers write
 *  the payload back with the code they have for SEI.  What cannot be carried is refused under the flag, LH264_E_UNSUPPORTED with a
 *  text that names the unit (lh264_parser_not_carried): a unit of type 1 or 5 that is not handed to the model (it arrives before its
 *  parameter sets, or is a redundant picture), a unit with the forbidden bit set; a slice whose header does not parse (an unknown PPS)
 *  or whose data stops parsing halfway is refused with the parser's text, as without the flag.  B, SP and SI slices, FMO and
 *  interlace stay refused; trailing zero bytes behind a CABAC slice stay as they are.
 *  (b) LOST SLICES: a picture with macroblocks no slice covers no longer refuses the stream: such a macroblock has no symbols, and
 *  its entry of the nnz image is the KEEP entry (see lh264_ctx_index_chains_keep), which is what the restorers hold there.
 * Without the flag nothing changes; a stream without such units and with whole pictures gets the same bytes with it as without -
 * except one that changes its picture size, where PAST and KEEP start from nothing under the flag as they do in the restorers. */
#define LH264_COMPRESS_ESCAPES 1u
#define LH264_COMPRESS_TOLERANT 2u
typedef struct lh264_compress_opts { uint32_t struct_bytes; uint32_t reserved; uint64_t segment_mbs; } lh264_compress_opts_t;
int lh264_compress_batch_opts (const uint8_t* const* data, const size_t* len, int n, int threads, const lh264_compress_opts_t* opts, lh264_compressed_t** out);
int lh264_compress_batch_devices_opts (const uint8_t* const* data, const size_t* len, int n, int threads, const int* devices, int n_devices,
                                       const lh264_compress_opts_t* opts, lh264_compressed_t** out);
/* in how many segments the stream was coded (1: whole; 0: not coded), and the decisions coded into a tag's list, summed over them */
int lh264_compressed_segments (const lh264_compressed_t* c);
uint64_t lh264_compressed_decisions (const lh264_compressed_t* c, int tag);
/* what the buffers lh264_compress_batch keeps on the current device hold after a call: device memory (with the most the long streams of
 * the last call held beside them) and page-locked host memory, in bytes */
int lh264_compress_arena_bytes (size_t* device, size_t* pinned);
int lh264_compressed_status (const lh264_compressed_t* c);
const char* lh264_compressed_error (const lh264_compressed_t* c);
const uint8_t* lh264_compressed_main (const lh264_compressed_t* c, size_t* len);
const uint8_t* lh264_compressed_tag (const lh264_compressed_t* c, int tag, size_t* len);     /* NULL: the stream does not exist */
int lh264_compressed_pictures (const lh264_compressed_t* c);
void lh264_compressed_free (lh264_compressed_t* c);
void lh264_compress_release (void);       /* frees the device and page-locked buffers lh264_compress_batch keeps between calls */

/* ---- batches of independent streams on the host cores (streams are independent, one thread each) --
 * lh264_parse_batch: n Annex-B files -> n parsers (lh264_parser_feed_file each), `threads` worker threads (0 = one per
 * hardware thread).  parsers_out[i] is always a valid handle to destroy; its error text tells whether the stream parsed.
 * lh264_pip_restore_batch: n restores as lh264_pip_restore, item by item; item.status receives the return code. */
int lh264_parse_batch (const uint8_t* const* data, const size_t* len, int n, int threads, lh264_parser_t** parsers_out);
/* the same work with every picture released as soon as it is complete (what a pipeline does once the records are on their way
 * to the device): pictures_out[i] = pictures parsed of stream i.  The steady-state throughput probe of the front end. */
int lh264_parse_batch_discard (const uint8_t* const* data, const size_t* len, int n, int threads, int64_t* pictures_out);
typedef struct lh264_restore_item {
  const uint8_t* main_stream; size_t main_len;
  const uint8_t* const* tags; const size_t* tag_len; int32_t n_tags;
  int32_t status;                 /* out: LH264_OK / LH264_E_*                       */
  uint8_t* out; size_t out_cap;   /* caller's buffer                                 */
  size_t out_len;                 /* out: restored size (or the size needed)         */
} lh264_restore_item_t;
int lh264_pip_restore_batch (lh264_restore_item_t* items, int n, int threads);

/* ---- restore direction on the device (csrc/lh264_restore.hip) ------------------------------------------------------------
 * lh264_pip_restore_batch_device: the same n restores, with the same status, out and out_len per item as lh264_pip_restore_batch
 * (LH264_E_ARG with out_len = the size needed included), synchronously on the current device.  Host pass 1 reads the slice headers
 * of each default stream (`threads` host threads, 0 = all); one single-wave workgroup per stream runs the adaptive decode and the
 * macroblock writer of each slice - the CAVLC writer; the CABAC writer where the caller asks for it (LH264_RESTORE_CABAC_DEVICE),
 * otherwise a stream with a CABAC slice is restored by the host beside the kernel -; host pass 2 splices the slices' bits behind
 * their headers.  path_out[i] (may be NULL) tells how item i was restored.  Without a device: LH264_E_NODEVICE, the items untouched.
 * Device and page-locked buffers are kept between calls (lh264_restore_release frees them); concurrent calls on one device are
 * serialised by a lock. */
#define LH264_RESTORE_PATH_DEVICE   0   /* restored by the kernel                                                               */
#define LH264_RESTORE_PATH_HOST     1   /* the stream has CABAC slices (and no LH264_RESTORE_CABAC_DEVICE): the host restore      */
#define LH264_RESTORE_PATH_FALLBACK 2   /* the device path stopped (capacity, corrupt input, I_PCM without samples): lh264_pip_restore */
int lh264_pip_restore_batch_device (lh264_restore_item_t* items, int n, int threads, int32_t* path_out);
/* the same with options; lh264_pip_restore_batch_device behaves as this call with zeroed flags.  LH264_RESTORE_CABAC_DEVICE: streams
 * with CABAC slices are planned like the others (per slice: a stream may change between CAVLC and CABAC with its PPS) and the batch
 * runs the kernel instance that has the CABAC writer (9.3.2 - 9.3.4) beside the CAVLC one; LH264_RESTORE_PATH_HOST is then reported
 * for no item.  Opt-in: which side is faster for a batch is in DESIGN.md 4.5.  opts == NULL: zeroed flags and threads = 0.  A
 * struct_bytes this library does not know or unknown flag bits: LH264_E_ARG, before the device is looked at. */
#define LH264_RESTORE_CABAC_DEVICE 1u   /* streams with CABAC slices take the kernel too */
typedef struct lh264_restore_opts { uint32_t struct_bytes; int32_t threads; uint32_t flags; } lh264_restore_opts_t;
int lh264_pip_restore_batch_device_opts (lh264_restore_item_t* items, int n, const lh264_restore_opts_t* opts, int32_t* path_out);
void lh264_restore_release (void);
/* milliseconds of the last lh264_pip_restore_batch_device call in this process: ms[0] host pass 1 and staging, ms[1] the device
 * stage (upload, kernel, download; the CABAC streams on the host meanwhile), ms[2] the kernel alone (HIP events), ms[3] host pass 2
 * and the fallbacks */
int lh264_restore_last_timing (double* ms);
/* the kernel's code (csrc/lh264_restore.hip) stepped on the host threads over host memory, with the same plan, capacities and
 * results as lh264_pip_restore_batch_device: a check of the device chain where no device is present; not a restore path */
int lh264_debug_restore_cpu (lh264_restore_item_t* items, int n, int threads, int32_t* path_out);
int lh264_debug_restore_cpu_opts (lh264_restore_item_t* items, int n, const lh264_restore_opts_t* opts, int32_t* path_out);
/* the restore kernel's adaptive-probability update ON THE DEVICE, alone: out[i] = the probability word (c0 bits 0-9, c1 bits 10-19,
 * prob bits 20-27) that follows words[i] after the decision bits[i].  Its division by a reciprocal exists in device code only, so
 * lh264_debug_restore_cpu never steps it; a test runs every reachable pair of counts through this.  Without a device: LH264_E_NODEVICE */
int lh264_debug_dp_update (const uint32_t* words, const uint8_t* bits, uint32_t* out, int n);

/* ---- the decode direction behind one call (csrc/lh264_decode.hip) -------------------------------------------------------------
 * n independent Annex-B files in host memory -> per stream its pictures in decode order (= output order: I and P slices only, as in
 * the reference), each cropped to the SPS window and tightly packed - LH264_FMT_I420: w*h Y, then w/2 * h/2 Cb, then Cr;
 * LH264_FMT_NV12: Y, then Cb / Cr interleaved - one behind the other with nothing between them: in I420 exactly the file the
 * reference's console application writes (h264dec.cpp Write2File).  offset counts from the stream's first byte; a stream may change
 * resolution, width / height are per picture.
 * The work runs in ROUNDS: every stream that takes part contributes its next round_pictures pictures at most, one
 * lh264_recon_chains launch reconstructs them (a chain per stream) into a per-stream pool of padded pictures (round_pictures + the
 * references the parser's DPB still holds), a pack kernel crops them into the round's output buffer, and the download runs on a
 * second HIP stream while the host threads (`threads`, 0 = all) parse and stage the next round: host and device memory follow the
 * round, not the streams' length.  group_mbs bounds the macroblocks of one round (streams wait their turn in the order given).
 * A reference slot a picture does not fill, or whose picture is not held any more, holds a picture of 128s: what a stream that has
 * lost its references reads there is defined and the same on every run.
 * opts->conceal (LH264_CONCEAL_*, the reference's ERROR_CON_IDC values; 0 and the 40-byte struct of before: off): a picture with
 * macroblocks no slice covers does not stop its stream; they are concealed as the reference's decoder does it - copied from the
 * picture decoded before (128s where there is none, and for an IDR picture under LH264_CONCEAL_SLICE_COPY), under the MV_COPY methods
 * moved by the mean vector of the received macroblocks - and lh264_decoded_concealed counts them per picture.  One rule differs from
 * the reference: the edge between a received and a concealed macroblock is not filtered (the reference filters it against what its
 * picture buffer held before).  The FREEZE methods withhold pictures until the first whole IDR picture: they are
 * decoded and not delivered.  LH264_CONCEAL_* values the call does not provide (the FRAME_COPY pair): LH264_E_ARG.  A slice that stops
 * parsing with an error and whole lost pictures are treated as without the option; a slice NAL unit cut short whose bits still parse
 * as a shorter slice is a shorter slice, and the macroblocks behind it are concealed.  The stream's last picture is delivered concealed
 * like any other (the reference's end-of-stream drain drops a damaged last picture).
 * Every out[i] is a handle to free.  A failure stays with its stream: LH264_E_UNSUPPORTED with the text of the front end for syntax it
 * does not parse; a picture with macroblocks no slice covers (unless opts->conceal), an incomplete slice or a NAL unit that does not parse
 * stops the stream THERE - the pictures in front of it are delivered and valid, the text names the picture.  A stream without a
 * picture and without an error is LH264_OK with no pictures.
 * sink: the handles keep no bytes; the sink is called with runs of consecutive pictures of one stream (pics[k].offset as above,
 * bytes = the first picture's first byte), in order within a stream, never from two threads at once, bytes valid for the call only;
 * a non-zero return stops that stream (LH264_E_ARG, text "sink").
 * The bytes do not depend on threads, round_pictures, group_mbs, the sink or on which other streams share the batch.
 * Digests (LH264_DECODE_SHA1_*): the SHA-1 of every delivered picture's bytes, and / or of all delivered pictures of the stream one
 * behind the other - for I420 the number the reference's decoder test keeps per stream (test/api/decoder_test.cpp) - computed on the
 * device from the round's packed buffer (sha1_spans_kernel), in every output mode.  A withheld picture has no index and no digest, a
 * concealed picture is hashed as delivered, a stream that stops at picture k has the digests of the pictures in front of it and a
 * stream digest over exactly their bytes, a stream without pictures the SHA-1 of the empty message.  With LH264_DECODE_NO_PICTURES
 * nothing is downloaded or kept: lh264_decoded_picture still describes every picture, lh264_decoded_bytes / _bytes_dev give NULL and
 * length 0.  The digests do not depend on threads, round_pictures, group_mbs, the output mode or the batch either.
 * opts->parse = LH264_PARSE_DEVICE (opt-in; struct_bytes 40 and 48 mean host): the host walks headers only (NAL split, unescape, SPS / PPS /
 * slice header, reference lists, marking, picture boundaries) and per round the payloads of the CAVLC slices and one task per slice go
 * to the device instead of records and coefficient lists; slice_parse_kernel writes the records and dequantised coefficients where
 * recon_chain_kernel reads them, and its 12 bytes per slice come down before the round's pictures are picked: from them the host fills
 * in n_mbs and coverage and applies the same rules as ever.  Per stream: host from the start with opts->conceal; host for a picture
 * with CABAC slices and for good behind the first of them; a round in which a slice of the stream gets a status (syntax the host fails
 * on, a slice that runs into the next one) is parsed again by the host parser, and the stream stays with it.  Pictures, statuses, texts,
 * digests and the stop-there position do not depend on parse.  lh264_decoded_parse_path tells the route.
 * opts->parse_flags = LH264_PARSE_FLAG_CABAC together with LH264_PARSE_DEVICE (struct_bytes 40 and 48: not read): CABAC slices become
 * tasks as well, in the same parse arena and with the same 12 bytes per slice coming down; slice_parse_cabac_kernel walks them, on the
 * same stream and ahead of the same synchronisation as slice_parse_kernel.  The stream then stays on the device route through CABAC
 * pictures; conceal and a status from either kernel send it to the host parser as before.  Without the flag nothing changes.
 * opts->scale_log2 = s in {1, 2, 3} (the 64-byte struct; struct_bytes 40, 48 and 56: not read, 0): REDUCED-SIZE pictures, averaged on the
 * device by decode_pack_scaled_kernel in place of the crop-and-copy kernel.  B = 1 << s.  For a picture whose cropped window is w x h
 * (both even), cw = w / 2 and ch = h / 2: the delivered chroma size is ocw = ceil (cw / B), och = ceil (ch / B), the delivered luma size
 * ow = 2 * ocw, oh = 2 * och (both even, so I420 / NV12 stay well formed).  Delivered luma sample (X, Y) =
 * (sum + (1 << (2*s - 1))) >> (2*s), where sum runs over the B x B window samples at x = min (X*B + i, w - 1), y = min (Y*B + j, h - 1),
 * 0 <= i, j < B; Cb and Cr: the same rule on their cw x ch planes.  Coordinates are clamped to the cropped window, never to the padded
 * picture: what lies right of and below the window enters no mean.  The planes are averaged independently; chroma siting is NOT
 * modelled (a luma sample and the chroma sample over it do not cover the same area of the picture exactly).  Packing is as at scale 0
 * with ow and oh in place of w and h, pictures tight one behind the other; lh264_decoded_pic_t width / height / bytes / offset describe
 * what is delivered, lh264_decoded_picture_source_size gives the window before scaling.  QCIF at s = 3: 22 x 18, 594 bytes.  The round's
 * output buffers, the download, the handles, the sink, DEVICE_OUT and the digests all work on the delivered bytes; withheld pictures
 * stay withheld, concealment and the parse routes are as at scale 0.  scale_log2 = 0 launches and delivers what the call did before.
 * opts->pick = LH264_PICK_INTRA or LH264_PICK_IDR (the 72-byte struct; struct_bytes up to 64: not read, LH264_PICK_ALL): only the SELECTED
 * pictures are decoded and delivered, in decode order - INTRA: every picture that has at least one slice and whose slices are all I
 * slices; IDR: the pictures whose slices are IDR slices.  Such a picture depends on no other, so each is byte for byte that picture of
 * a LH264_PICK_ALL call with the same format, scale and output mode.  Offsets, the handles, the sink (first_picture counts delivered
 * pictures), DEVICE_OUT, NO_PICTURES and both kinds of digest work on the delivered pictures only; lh264_decoded_picture_index gives a
 * delivered picture's number among all pictures of the stream.  Of an unselected picture the front end walks the headers (NAL split,
 * parameter sets, slice headers, reference marking, picture boundaries) and never looks at its slice data: no macroblock layer runs for
 * it on the host, it is no task for the parse kernels and has no records, coefficients, pool slot, job or pack job
 * (lh264_decoded_parsed_slices counts what was parsed).  The selected pictures' slice data is parsed by the host threads, or under
 * LH264_PARSE_DEVICE by the kernels with the same fallback rules.  A failure in the header walk stops the stream there, as ever; a selected
 * picture the full decode would refuse (uncovered macroblocks, an incomplete slice, a slice that does not parse) stops the stream at
 * that picture with the same text, the selected pictures in front of it delivered.  DAMAGE INSIDE THE SLICE DATA OF AN UNSELECTED PICTURE
 * IS NEITHER SEEN NOR REPORTED: a stream that LH264_PICK_ALL stops at such a picture is decoded to its end here.  A selected picture
 * references nothing, so each is a chain of its own in lh264_recon_chains (its job carries LH264_JOB_NO_EXPAND, its reference slots
 * point at the picture of 128s, its pool slot is free again behind its round): a stream spreads over as many workgroups as it has
 * selected pictures in the round (lh264_decode_last_chains).  pick other than LH264_PICK_ALL together with conceal is LH264_E_ARG:
 * concealment copies from the picture decoded before, which is not decoded here.
 * opts->out_width = OW, opts->out_height = OH (the 88-byte struct; struct_bytes up to 72: not read, 0, 0): PICTURES OF ONE GIVEN SIZE.
 * Every delivered picture of every stream is OW x OH (both even, 2..4096), resampled from its cropped window by an exact, integer area
 * average on the device: decode_pack_resized_kernel takes the copy kernel's place in the round.  Each plane is resampled on its own, the
 * luma plane from the w x h window to OW x OH, Cb and Cr from w/2 x h/2 to OW/2 x OH/2.  For one plane of w x h window samples p[y][x]
 * delivered as ow x oh: the horizontal weight of source column x for delivered column X is
 * wx (X, x) = max (0, min ((x+1)*ow, (X+1)*w) - max (x*ow, X*w)) - non-zero only for x in floor (X*w / ow) .. floor (((X+1)*w - 1) / ow),
 * ow for every column strictly inside that span, the weights of one X sum to w; the vertical weight wy (Y, y) is the same with h and oh.
 * S = the sum over y, x of wy (Y, y) * wx (X, x) * p[y][x], D = w*h, delivered sample (X, Y) = floor ((2*S + D) / (2*D)): round half up,
 * in exact integers (S is kept in 64 bits: exact for every window the front end delivers).  No coordinate leaves the window: nothing
 * right of or below it, and nothing of the padded picture, enters a mean.  The aspect ratio is NOT kept (a plain stretch); chroma siting
 * is not modelled, as at scale_log2.  ow == w and oh == h gives the window itself; w = B*ow and h = B*oh, B in 2 / 4 / 8, gives the
 * scale_log2 means byte for byte (QCIF at 88 x 72, 44 x 36, 22 x 18); a larger size than the window repeats samples and blends the seams.
 * Packing is as ever with OW, OH in place of w, h.  lh264_decoded_pic_t width / height / bytes / offset describe what is delivered,
 * lh264_decoded_picture_source_size gives the window.  The round's output buffers, the download, the handles, the sink, DEVICE_OUT and
 * the digests work on the delivered bytes (lh264_decode_arena_bytes follows them: more than at full size where OW x OH is larger than
 * the window); withheld pictures stay withheld; format, conceal, parse and pick act on what is decoded as without a size.  0, 0 launches
 * and delivers what the call did before.
 * Arguments are checked first (LH264_E_ARG: a struct_bytes this library does not know, one of out_width / out_height 0 and the other not, either of
 * them odd or above 4096, a size together with scale_log2, reserved4 or reserved5 not 0 in the 88-byte struct, a parse value that is not defined, a parse_flags bit that is not defined or
 * LH264_PARSE_FLAG_CABAC with LH264_PARSE_HOST, scale_log2 above 3 or reserved2 not 0 in the 64-byte struct, pick above 2, reserved3 not 0 or pick with conceal in the 72-byte struct, a format out of range, a flag bit that is not
 * defined, sink together with LH264_DECODE_DEVICE_OUT, LH264_DECODE_NO_PICTURES without a digest flag or together with
 * LH264_DECODE_DEVICE_OUT or a sink, n < 0), then the device (LH264_E_NODEVICE); out is untouched in both cases.  Device and page-locked buffers
 * are kept between calls, per device (lh264_decode_release frees them); concurrent calls on one device are serialised by a lock. */
#define LH264_FMT_I420 0
#define LH264_FMT_NV12 1
#define LH264_DECODE_DEVICE_OUT 1u   /* the pictures stay in device memory owned by the handle */
/* (bits 2u and 16u are not defined and stay LH264_E_ARG, as every other bit: callers and tests of the library before the digests
 * rely on 2u being refused) */
#define LH264_DECODE_SHA1_PICTURES 4u /* a digest per delivered picture, of the bytes the call delivers (I420 or NV12 as asked) */
#define LH264_DECODE_SHA1_STREAM 8u   /* one digest of all delivered pictures of the stream in order: the reference's table for I420 */
#define LH264_DECODE_NO_PICTURES 32u  /* digests only: nothing is downloaded or kept */
typedef struct lh264_decoded lh264_decoded_t;
typedef struct lh264_decoded_pic { int32_t width, height, frame_num, idr; uint64_t offset, bytes; } lh264_decoded_pic_t;
typedef int (*lh264_decode_sink_fn) (void* user, int stream, int first_picture, int n_pictures,
                                     const lh264_decoded_pic_t* pics, const uint8_t* bytes, size_t len);
typedef struct lh264_decode_opts {
  uint32_t struct_bytes, format;        /* LH264_FMT_*                                                          */
  uint32_t flags;                       /* LH264_DECODE_*                                                       */
  uint32_t round_pictures;              /* pictures of one stream per launch at most; 0 = the default (8)       */
  uint64_t group_mbs;                   /* macroblocks of one round at most; 0 = the default (1,000,000)        */
  lh264_decode_sink_fn sink; void* user;
  uint32_t conceal;                     /* LH264_CONCEAL_*; 0 = off.  (struct_bytes up to `user`: off)          */
  uint32_t reserved0;                   /* (the tail padding of the 48-byte struct: callers of it left it undefined, it is not read) */
  uint32_t parse;                       /* LH264_PARSE_*; 0 = host.  (struct_bytes 40 and 48: host)             */
  uint32_t parse_flags;                 /* LH264_PARSE_FLAG_*; 0 = none.  (struct_bytes 40 and 48: not read)   */
  uint32_t scale_log2;                  /* 0 = full size; 1..3 = means of 2x2 / 4x4 / 8x8 blocks.  (struct_bytes up to 56: not read, 0) */
  uint32_t reserved2;                   /* 0                                                                    */
  uint32_t pick;                        /* LH264_PICK_*; 0 = every picture.  (struct_bytes up to 64: not read, 0) */
  uint32_t reserved3;                   /* 0                                                                    */
  uint32_t out_width, out_height;       /* 0, 0 = the stream's size (or its scale); else every delivered picture is out_width x out_height: both even, 2..4096, scale_log2 0.  (struct_bytes up to 72: not read, 0) */
  uint32_t reserved4, reserved5;        /* 0                                                                    */
} lh264_decode_opts_t;
#define LH264_DECODE_OPTS_BYTES_V1 40u  /* the struct before `conceal` was added: still accepted                 */
#define LH264_DECODE_OPTS_BYTES_V2 48u  /* the struct before `parse` was added: still accepted                   */
#define LH264_DECODE_OPTS_BYTES_V3 56u  /* the struct before `scale_log2` was added: still accepted, full size   */
#define LH264_DECODE_OPTS_BYTES_V4 64u  /* the struct before `pick` was added: still accepted, every picture     */
#define LH264_DECODE_OPTS_BYTES_V5 72u  /* the struct before `out_width` was added: still accepted, no size      */
#define LH264_PICK_ALL   0u             /* every picture of the stream (the default)                             */
#define LH264_PICK_INTRA 1u             /* the pictures that have a slice and whose slices are all I slices      */
#define LH264_PICK_IDR   2u             /* the pictures whose slices are IDR slices                              */
#define LH264_PARSE_HOST   0u           /* the host front end parses slice data (the default)                    */
#define LH264_PARSE_DEVICE 1u           /* CAVLC slice data is parsed by slice_parse_kernel, one wave per slice  */
#define LH264_PARSE_FLAG_CABAC 1u       /* with LH264_PARSE_DEVICE: CABAC slice data too, by slice_parse_cabac_kernel */
#define LH264_PARSE_PATH_HOST     0
#define LH264_PARSE_PATH_DEVICE   1
#define LH264_PARSE_PATH_FALLBACK 2
int lh264_decode_batch (const uint8_t* const* data, const size_t* len, int n, int threads,
                        const lh264_decode_opts_t* opts /* NULL = defaults */, lh264_decoded_t** out);
/* ---- RGB pictures, colour-converted on the device: lh264_decode_batch_ex -------------------------------------------------------------
 * The options above are frozen at 88 bytes; what comes after them travels in a struct of its own.  ext == NULL or ext->colour ==
 * LH264_COLOUR_YUV is lh264_decode_batch, byte for byte and launch for launch (lh264_decode_batch is this call with ext == NULL).
 * ORDER.  The conversion acts on the DELIVERED planes: first the window is copied, averaged (scale_log2) or resampled (out_width /
 * out_height) exactly as without colour, which gives ow x oh luma and ow/2 x oh/2 Cb and Cr samples; then every luma sample (X, Y) is
 * converted with the chroma sample (X >> 1, Y >> 1).  That is replication: chroma siting is NOT modelled, as everywhere else in this
 * call.  So the RGB bytes of a call are the function below applied to the I420 bytes of the same call made without colour.
 * STANDARD.  A matrix - BT.601: Kr = 299/1000, Kb = 114/1000; BT.709: Kr = 2126/10000, Kb = 722/10000; Kg = 1 - Kr - Kb - and a range,
 * limited (y0 = 16, sy = 255/219, sc = 255/224) or full (y0 = 0, sy = sc = 1).  As real numbers, with D = Cb - 128 and E = Cr - 128:
 *   R = sy*(Y - y0) + sc*2(1 - Kr)*E,   B = sy*(Y - y0) + sc*2(1 - Kb)*D,
 *   G = sy*(Y - y0) - sc*(2Kb(1 - Kb)/Kg)*D - sc*(2Kr(1 - Kr)/Kg)*E.
 * THE INTEGER FUNCTION (normative; what is delivered).  The five factors cy = sy, crv = sc*2(1 - Kr), cbu = sc*2(1 - Kb),
 * cgu = sc*2Kb(1 - Kb)/Kg, cgv = sc*2Kr(1 - Kr)/Kg are the exact rationals times 65536, rounded half up to integers: the table
 * LH264_COLOUR_FACTORS below, which the kernel, the host stepping and the documents all read (BT.601 full: crv = 91881; BT.601 limited:
 * cy = 76309).  In int32, `>>` an arithmetic shift, clip8 a clamp to 0..255:
 *   R = clip8 ((cy*(Y - y0) + crv*E + 32768) >> 16)
 *   G = clip8 ((cy*(Y - y0) - cgu*D - cgv*E + 32768) >> 16)
 *   B = clip8 ((cy*(Y - y0) + cbu*D + 32768) >> 16)
 * Every sum stays below 2^27 in magnitude; there are no floats anywhere.  Against the real-valued formula rounded half up and clipped it
 * differs by at most 1, in a small share of all (Y, Cb, Cr) triples (DESIGN.md section 4.6 has the count).
 * LAYOUTS.  LH264_COLOUR_RGB24: oh rows of ow pixels stored R, G, B - 3*ow*oh bytes, tight.  LH264_COLOUR_RGBP: three ow x oh planes,
 * R then G then B, tight.  Pictures lie one behind the other as ever; lh264_decoded_pic_t bytes / offset describe what is delivered
 * (twice I420's bytes), and the round's output buffers, the download, the handles, the sink, DEVICE_OUT, NO_PICTURES and both digests
 * work on those bytes.  Conceal, both parse routes, pick, scale_log2 and out_width / out_height act on what is decoded as without colour.
 * decode_pack_rgb_kernel takes the pack kernel's place in the round and writes the RGB bytes in one pass: no I420 intermediate.
 * WHICH STANDARD A STREAM GETS.  The front end reads the SPS VUI up to video_signal_type (aspect_ratio_info, overscan_info,
 * video_signal_type with video_full_range_flag, colour_description_present_flag and matrix_coefficients) and no further.  matrix =
 * LH264_MATRIX_AUTO: matrix_coefficients 1 gives BT.709; 5 or 6 give BT.601; 2 (unspecified), or no colour description, gives BT.601 -
 * the project's material is QCIF to SD conformance content; any other value stops the stream with LH264_E_UNSUPPORTED and a text that
 * names the value, at the first picture that carries it (a stream whose first SPS says so delivers nothing): a wrong colour is worse
 * than a refusal, and the caller can name a matrix.  range = LH264_RANGE_AUTO: video_full_range_flag decides; absent means limited.  A
 * named matrix or range overrides the stream's.  The standard is per picture (an SPS may change it inside a stream);
 * lh264_decoded_picture_colour tells what was applied to delivered picture idx: *matrix LH264_MATRIX_BT601 or _BT709, *full_range 0 or 1
 * (either may be NULL; LH264_E_ARG: a bad index, or a call without colour, which applied none).
 * LH264_E_ARG, checked before the device with out untouched, beside every case of lh264_decode_batch: a struct_bytes other than 24,
 * colour, matrix or range above 2, a reserved word that is not 0, matrix or range set while colour is LH264_COLOUR_YUV, colour together
 * with an opts->format other than LH264_FMT_I420. */
#define LH264_COLOUR_YUV   0u
#define LH264_COLOUR_RGB24 1u
#define LH264_COLOUR_RGBP  2u
#define LH264_MATRIX_AUTO  0u
#define LH264_MATRIX_BT601 1u
#define LH264_MATRIX_BT709 2u
#define LH264_RANGE_AUTO    0u
#define LH264_RANGE_LIMITED 1u
#define LH264_RANGE_FULL    2u
/* a standard in one byte, as the job tables carry it: bit 0 the matrix (0 BT.601, 1 BT.709), bit 1 the range (0 limited, 1 full);
 * LH264_COLOUR_FACTORS[that byte] = {cy, crv, cbu, cgu, cgv}, y0 = 16 where bit 1 is clear */
#define LH264_COLOUR_FACTORS { \
  { 76309, 104597, 132201, 25675, 53279 },   /* BT.601 limited */ \
  { 76309, 117489, 138438, 13975, 34925 },   /* BT.709 limited */ \
  { 65536,  91881, 116130, 22553, 46802 },   /* BT.601 full    */ \
  { 65536, 103206, 121609, 12276, 30679 } }  /* BT.709 full    */
typedef struct lh264_decode_ext {
  uint32_t struct_bytes;                /* 24                                                                   */
  uint32_t colour;                      /* LH264_COLOUR_*; 0 = the planes as lh264_decode_batch delivers them   */
  uint32_t matrix;                      /* LH264_MATRIX_*; 0 = what the stream's SPS says                       */
  uint32_t range;                       /* LH264_RANGE_*; 0 = what the stream's SPS says                        */
  uint32_t reserved0, reserved1;        /* 0                                                                    */
} lh264_decode_ext_t;
int lh264_decode_batch_ex (const uint8_t* const* data, const size_t* len, int n, int threads,
                           const lh264_decode_opts_t* opts /* NULL = defaults */, const lh264_decode_ext_t* ext /* NULL = no colour */, lh264_decoded_t** out);
int lh264_decoded_picture_colour (const lh264_decoded_t* d, int idx, uint32_t* matrix, int32_t* full_range);
/* ---- float RGB tensors, normalised on the device: lh264_decode_batch_ex2 ---------------------------------------------------------------
 * Both structs above are frozen; the sample words travel in a third.  sample == NULL, or type == LH264_SAMPLE_U8 with all six floats
 * +0.0 (every bit clear), is lh264_decode_batch_ex, byte for byte and launch for launch (lh264_decode_batch_ex is this call with NULL).
 * THE DEFINITION (normative).  A sample type is uint8 (the bytes of the calls above), float32, float16 or bfloat16.  With a float type,
 * element e of a delivered picture is a function of byte e of that picture in the same call made with LH264_SAMPLE_U8.  With c that
 * byte (0..255) and ch its channel (0 = R, 1 = G, 2 = B):
 *   v32 = fma ((float) c, mul[ch], add[ch])       one IEEE-754 binary32 fused multiply-add, round to nearest even
 *   LH264_SAMPLE_F32:  v32
 *   LH264_SAMPLE_F16:  v32 rounded to binary16, nearest even   (overflow gives infinity: there is no saturation)
 *   LH264_SAMPLE_BF16: v32 rounded to bfloat16, nearest even
 * mul[3] and add[3] are six binary32 values of the caller's.  Underflow is gradual in all three types: nothing is flushed to zero.  The
 * bits are what is defined, the sign of a zero included (fma (0, -1, +0.0) is +0.0, fma (0, -1, -0.0) is -0.0).
 * LAYOUT.  The uint8 call's with elements in place of bytes: LH264_COLOUR_RGB24 is oh rows of ow pixels stored R, G, B, LH264_COLOUR_RGBP
 * three ow x oh planes; elements are little-endian and tight; a picture is 3*ow*oh*es bytes, es = 4, 2, 2.  lh264_decoded_pic_t bytes /
 * offset describe what is delivered, and the round's output buffers, the download, the handles, the sink, DEVICE_OUT, NO_PICTURES, both
 * digests and lh264_decode_arena_bytes work on those bytes, as for RGB.  Conceal, both parse routes, pick, scale_log2, out_width /
 * out_height, matrix and range act as without a float type.  ow and oh are even, so every picture and every row of it begins at a
 * multiple of 4 bytes from the stream's first byte (of 8, in fact); the call checks that of every round's output offsets.
 * decode_pack_sample_kernel takes decode_pack_rgb_kernel's place in the round: the uint8 RGB never reaches memory.
 * LH264_E_ARG, checked before the device with out untouched, beside every case of the calls above: a struct_bytes other than 32, a type
 * above 3, LH264_SAMPLE_U8 with a float that is not +0.0, a float type with ext NULL or ext->colour == LH264_COLOUR_YUV, a mul or add
 * that is not finite.  lh264_decoded_sample_type: the LH264_SAMPLE_* of the call that made the handle (LH264_E_ARG: d NULL). */
#define LH264_SAMPLE_U8   0u
#define LH264_SAMPLE_F32  1u
#define LH264_SAMPLE_F16  2u
#define LH264_SAMPLE_BF16 3u
typedef struct lh264_decode_sample {
  uint32_t struct_bytes;                /* 32                                                                   */
  uint32_t type;                        /* LH264_SAMPLE_*                                                       */
  float    mul[3], add[3];              /* per channel R, G, B                                                  */
} lh264_decode_sample_t;
int lh264_decode_batch_ex2 (const uint8_t* const* data, const size_t* len, int n, int threads,
                            const lh264_decode_opts_t* opts /* NULL = defaults */, const lh264_decode_ext_t* ext /* NULL = no colour */,
                            const lh264_decode_sample_t* sample /* NULL = uint8 */, lh264_decoded_t** out);
int lh264_decoded_sample_type (const lh264_decoded_t* d);
/* ---- fitted views: a caller's crop, cover and letterbox: lh264_decode_batch_ex3 ----------------------------------------------------------
 * The three structs above are frozen; the view travels in a fourth.  view == NULL is lh264_decode_batch_ex2, byte for byte and launch for
 * launch (lh264_decode_batch_ex2 is this call with NULL).
 * THE DEFINITION (normative).  A view is applied per delivered picture, BEFORE any sizing.  Let w x h be the picture's cropped SPS window
 * (even, as ever).  All arithmetic below is in integers and `/` is floor.
 * CALLER'S CROP (optional): a rectangle {x, y, w, h} in window coordinates, all four even, x, y >= 0, w, h >= 2, x + w <= the window's
 * width, y + h <= its height.  With a crop the rectangle takes the window's place in every definition of the calls above: the copy, the
 * scale_log2 means (clamping is to the crop, never to what lies outside it), the resampling, colour and float.  Nothing outside the
 * rectangle enters any delivered sample.  w = h = 0 means no crop.  crops[i] is stream i's (n_crops = n), or crops[0] every stream's
 * (n_crops = 1).  A crop that does not fit a picture's window can only be known at that picture (a stream may change size): it stops the
 * stream there with LH264_E_ARG and a text that names the picture, the rectangle and the window; the pictures in front of it are delivered.
 * FIT (needs out_width / out_height = OW x OH); w, h below are the window after the caller's crop.
 *   LH264_FIT_STRETCH: the whole window is resampled to OW x OH, as without a view.
 *   LH264_FIT_COVER: the largest centred sub-rectangle of the window with the output's aspect, stretched to OW x OH.
 *     w*OH > h*OW: sh = h, sw = max (2, 2 * ((h*OW + OH) / (2*OH)));  w*OH < h*OW: sw = w, sh = max (2, 2 * ((w*OH + OW) / (2*OW)));
 *     equality: the whole window.  sx = 2 * ((w - sw) / 4), sy = 2 * ((h - sh) / 4).  The source is {sx, sy, sw, sh} inside the window,
 *     resampled to OW x OH by the rule of out_width / out_height.
 *   LH264_FIT_CONTAIN: the whole window resampled into the largest centred even rectangle of the output, the rest filled.
 *     w*OH > h*OW: dw = OW, dh = max (2, 2 * ((h*OW + w) / (2*w)));  w*OH < h*OW: dh = OH, dw = max (2, 2 * ((w*OH + h) / (2*h)));
 *     equality: the whole output.  dx = 2 * ((OW - dw) / 4), dy = 2 * ((OH - dh) / 4).  Luma sample (X, Y) of the delivered OW x OH plane
 *     is the resampling of the w x h window to dw x dh at (X - dx, Y - dy) where that lies in [0, dw) x [0, dh); elsewhere it is fill_y.
 *     Cb and Cr: the same rule with every quantity halved, and fill_cb, fill_cr.
 * Every rectangle is even, at least 2 x 2 and inside the window or the output.  The aspect ratio is kept to the nearest even sample, NOT
 * exactly.  176 x 144 to 224 x 224: cover reads {16, 0, 144, 144}, contain writes {0, 20, 224, 184}; 1920 x 1080: {420, 0, 1080, 1080}
 * and {0, 48, 224, 126}.  lh264_view_rects is this rule and needs no device.
 * Colour and float types act on the DELIVERED planes exactly as without a view: the RGB bytes of a view call are the integer function
 * applied to the I420 bytes of the same call without colour, bars included (a bar pixel is the conversion of fill_y, fill_cb, fill_cr),
 * the float elements the fma of those bytes.  Every rectangle is even, so a 2x2 quad is wholly picture or wholly bar.
 * Crop and cover narrow the source rectangle of the pack jobs and launch the kernels of the calls above; contain launches their placed
 * siblings (decode_pack_placed_kernel, decode_pack_rgb_placed_kernel, decode_pack_sample_placed_kernel), which write the bars by plain
 * stores.  Offsets, handles, the sink, DEVICE_OUT, NO_PICTURES, both digests and the arena follow the delivered bytes as ever; conceal,
 * both parse routes, pick, format, scale_log2, colour and the sample type act as without a view.  lh264_decoded_picture_source_size
 * keeps returning the SPS window; lh264_decoded_picture_view gives the source rectangle in window coordinates and the destination
 * rectangle in the delivered picture (either may be NULL; without a view {0, 0, w, h} and {0, 0, ow, oh}; LH264_E_ARG: a bad index).
 * LH264_E_ARG, checked before the device with out untouched, beside every case of the calls above: a struct_bytes other than 32, fit
 * above 2, a fit other than stretch without out_width / out_height, fill non-zero without LH264_FIT_CONTAIN or with bits 24..31 set, a
 * reserved word that is not 0, n_crops not 0, 1 or n, n_crops != 0 with crops NULL, a crop with a negative or odd member, a crop with
 * exactly one of w, h zero. */
typedef struct lh264_rect { int32_t x, y, w, h; } lh264_rect_t;
#define LH264_FIT_STRETCH 0u
#define LH264_FIT_COVER   1u
#define LH264_FIT_CONTAIN 2u
typedef struct lh264_decode_view {
  uint32_t struct_bytes;                /* 32                                                                   */
  uint32_t fit;                         /* LH264_FIT_*                                                          */
  uint32_t fill;                        /* fill_y | fill_cb << 8 | fill_cr << 16; read under LH264_FIT_CONTAIN only */
  uint32_t n_crops;                     /* 0: none; 1: crops[0] for every stream; n: crops[i] for stream i      */
  const lh264_rect_t* crops;
  uint32_t reserved0, reserved1;        /* 0                                                                    */
} lh264_decode_view_t;
int lh264_decode_batch_ex3 (const uint8_t* const* data, const size_t* len, int n, int threads,
                            const lh264_decode_opts_t* opts /* NULL = defaults */, const lh264_decode_ext_t* ext /* NULL = no colour */,
                            const lh264_decode_sample_t* sample /* NULL = uint8 */, const lh264_decode_view_t* view /* NULL = none */, lh264_decoded_t** out);
int lh264_decoded_picture_view (const lh264_decoded_t* d, int idx, lh264_rect_t* src, lh264_rect_t* dst);
/* ---- motion fields: vectors, references, macroblock data: lh264_decode_batch_ex4 --------------------------------------------------------
 * The four structs above are frozen; the fields travel in a fifth.  motion == NULL or fields == 0 is lh264_decode_batch_ex3, byte for
 * byte and launch for launch (lh264_decode_batch_ex3 is this call with NULL).
 * THE DEFINITION (normative).  For every DELIVERED picture of a stream two blocks, which cover the CODED picture of mb_w x mb_h
 * macroblocks, not the cropped window; nothing in scale_log2, out_width / out_height, the view, colour or the sample type touches them.
 * MOTION BLOCK: int16, little-endian, three planes of (4*mb_h) x (4*mb_w), plane after plane: 96 bytes a macroblock.  Cell (X, Y)
 * belongs to macroblock (X >> 2, Y >> 2) and to its raster 4x4 block b = (Y & 3) * 4 + (X & 3).
 *   planes 0, 1: dx, dy = mv[b][0], mv[b][1] of the macroblock's record (lh264_mb_t): quarter-pel, the final vector, for P_Skip the
 *     inferred one.  A record with LH264_MB_CONCEAL gives mv[0] in all sixteen cells, the vector the reconstruct kernel reads (the front
 *     end fills all sixteen vectors of such a record with that vector and its ref_idx with 0, so both readings agree on its records).
 *   plane 2: `back`, how many pictures back in decode order the cell predicts from: lh264_decoded_picture_index of this picture minus
 *     that of the reference picture (withheld and unselected pictures count).  r = ref_idx[(b >> 3) * 2 + ((b & 3) >> 1)], slot =
 *     slices[slice_id].ref_slot[r], the picture is the one behind job reference `slot`.  back = -1 where that names no decoded picture:
 *     r or slot outside 0..15, a slice_id past the picture's table, a slot past the job's references, a reference the decoder no longer
 *     holds, the picture of 128s (the P pictures in front of a lost first IDR; a concealed macroblock whose source is the 128 picture).
 *   A cell of an intra macroblock (mb_type & LH264_MB_INTRA), of an uncovered one (mb_type 0) and of a record whose kind below is 0 is
 *   0, 0, 0 whatever the record holds.
 * MACROBLOCK BLOCK: uint8, eight planes of mb_h x mb_w: 8 bytes a macroblock.
 *   [0] kind, the first of these that mb_type has a bit of: 1 I4x4, 2 I8x8, 3 I16x16, 4 I_PCM, 5 P_Skip, 6 P16x16, 7 P16x8, 8 P8x16,
 *       9 P8x8, 10 P8x8ref0; 0: none of them (not covered)        [1] qp_y        [2] cbp
 *   [3] flags: bit 0 LH264_MBF_T8x8, bit 1 concealed (LH264_MB_CONCEAL)        [4..7] sub_type[0..3] for kinds 9 and 10, else 0
 * Per stream the motion blocks of its delivered pictures lie tight one behind the other in one buffer, the macroblock blocks in a
 * second; every block begins at a multiple of 8 bytes.  lh264_decoded_picture_motion gives a picture's geometry and offsets: crop_x,
 * crop_y place the delivered window in the coded picture, so fields line up with pixels (luma sample (x, y) of the window lies in cell
 * ((crop_x + x) >> 2, (crop_y + y) >> 2)).  lh264_decoded_motion gives the two buffers in host memory, lh264_decoded_motion_dev in device
 * memory under LH264_DECODE_DEVICE_OUT (each gives NULL in the other mode; any out pointer may be NULL), lh264_decoded_motion_copy_dev
 * copies both into the caller's device memory (either destination may be NULL; cap >= the length), complete on return.  All of them
 * return LH264_E_ARG on a handle whose call asked for no fields, and on a bad index.
 * With fields the pictures are delivered exactly as without them, in every mode; a sink receives the pictures, the fields stay on the
 * handle.  conceal, both device parse routes, pick (every delivered picture is intra: all cells 0), round_pictures and group_mbs act as
 * ever; withheld pictures deliver no fields; a stream that stops delivers the fields of the pictures in front of the stop.
 * MOTION ONLY: with fields, LH264_DECODE_NO_PICTURES is accepted without a digest flag, and together with LH264_DECODE_DEVICE_OUT (the
 * fields then stay on the device); with a sink it stays LH264_E_ARG.  Without a digest flag no picture pool is used and no reconstruct,
 * pack or digest kernel is launched: lh264_decode_last_chains reports 0 rounds, chains and jobs, the picture records are those of the
 * digests-only call.  decode_pack_motion_kernel gathers the records where the round's parse or upload left them, in front of the
 * reconstruct launch.
 * LH264_E_ARG, checked before the device with out untouched, beside every case of the calls above: a struct_bytes other than 16, fields
 * above 1, a reserved word that is not 0. */
#define LH264_MOTION_FIELDS 1u
typedef struct lh264_decode_motion {
  uint32_t struct_bytes;                /* 16                                                                   */
  uint32_t fields;                      /* 0: none (the call is lh264_decode_batch_ex3); LH264_MOTION_FIELDS    */
  uint32_t reserved0, reserved1;        /* 0                                                                    */
} lh264_decode_motion_t;
typedef struct lh264_decoded_motion { int32_t mb_w, mb_h, crop_x, crop_y; uint64_t motion_offset, info_offset; } lh264_decoded_motion_t;
int lh264_decode_batch_ex4 (const uint8_t* const* data, const size_t* len, int n, int threads,
                            const lh264_decode_opts_t* opts /* NULL = defaults */, const lh264_decode_ext_t* ext /* NULL = no colour */,
                            const lh264_decode_sample_t* sample /* NULL = uint8 */, const lh264_decode_view_t* view /* NULL = none */,
                            const lh264_decode_motion_t* motion /* NULL = no fields */, lh264_decoded_t** out);
int lh264_decoded_picture_motion (const lh264_decoded_t* d, int idx, lh264_decoded_motion_t* out);
int lh264_decoded_motion (const lh264_decoded_t* d, const int16_t** motion, size_t* motion_bytes, const uint8_t** info, size_t* info_bytes);
int lh264_decoded_motion_dev (const lh264_decoded_t* d, const int16_t** motion, size_t* motion_bytes, const uint8_t** info, size_t* info_bytes);
int lh264_decoded_motion_copy_dev (const lh264_decoded_t* d, void* motion_dst_dev, size_t motion_cap, void* info_dst_dev, size_t info_cap);
/* the last call's decode_pack_motion_kernel launches in this process: *ms their milliseconds on the device (between events around each
 * launch), *bytes the field bytes they wrote (104 a macroblock).  Either may be NULL; 0, 0 after a call without fields */
int lh264_decode_last_motion (double* ms, unsigned long long* bytes);
/* ---- the pictures asked for by number, with their reference chains: lh264_decode_batch_ex5 ----------------------------------------------
 * The five structs above are frozen; the selection travels in a sixth.  select == NULL or n_selects == 0 is lh264_decode_batch_ex4,
 * byte for byte and launch for launch (lh264_decode_batch_ex4 is this call with NULL).
 * THE RULE (normative).  Pictures are numbered in decode order from 0, as lh264_decoded_picture_index numbers them (withheld and
 * unselected pictures count).  For one stream with the set Q of requested numbers:
 *   ENTRY pictures are picture 0 and every IDR picture.  A non-IDR picture whose slices are all I slices is NOT an entry: a later P
 *     picture may reference across it.  entry (r) is the largest entry picture <= r.
 *   NEEDED pictures are the union over r in Q of entry (r) .. r.  A RUN is a stretch of needed pictures that starts at an entry and
 *     ends in front of the next needed entry.
 *   needed and requested: decoded and DELIVERED.
 *   needed and not requested: decoded and RECONSTRUCTED ONLY - a pool slot and a reconstruct job, no pack job, no record, no bytes, no
 *     digest, no fields.
 *   not needed, at or before the last requested picture: walked by its headers only (NAL split, parameter sets, slice headers,
 *     reference marking, picture boundaries).  Its slice data is never looked at: no records, no slot, no job, exactly like an
 *     unselected picture under opts->pick.
 *   BEHIND THE LAST REQUESTED PICTURE THE STREAM ENDS: nothing more of it is read.  The end of that picture is found as always, so the
 *     header of the next access unit may be seen.  If every requested picture that exists was delivered the status is LH264_OK.
 *   A requested number at or beyond the stream's picture count delivers nothing and is no error: lh264_decoded_picture_index tells
 *     what arrived.
 * EVERY DELIVERED PICTURE IS BYTE FOR BYTE THAT PICTURE OF THE LH264_PICK_ALL CALL with the same format, scale, size, view, colour and
 * sample type.  Offsets, the handles, the sink (first_picture counts delivered pictures), DEVICE_OUT, NO_PICTURES and both kinds of
 * digest work on the delivered pictures only.  The fields of a delivered picture (lh264_decode_batch_ex4) are those of the full call,
 * `back` included: it counts pictures of the stream, not delivered ones.
 * FAILURES.  A failure of the header walk in front of the last requested picture stops the stream there, as ever, with the same
 * `picture N: text`.  A needed picture the full call would refuse (uncovered macroblocks, an incomplete slice, a slice that does not
 * parse, a crop that does not fit, a matrix without a conversion) stops the stream at that picture with the full call's code and text:
 * the refusals are checked on every picture of a run, as the full call checks them on every picture.  The requested pictures in front
 * of a stop are delivered.  DAMAGE INSIDE THE SLICE DATA OF A PICTURE THAT IS NOT NEEDED, OR ANYWHERE BEHIND THE LAST REQUESTED PICTURE,
 * IS NEITHER SEEN NOR REPORTED: a stream that the full call stops at such a place is decoded to its last requested picture here.
 * The slice data of the needed pictures is parsed by the host threads, or under LH264_PARSE_DEVICE by the kernels, on the paths and
 * with the fallback rules of opts->pick.  Within a round every run that begins at an IDR picture is a chain of its own in the
 * lh264_recon_chains launch (lh264_decode_last_chains): its first picture references nothing and its slots were free when the round
 * began, so two runs of one stream in one round are independent; a run that spans rounds goes on as the stream's chain in the next.
 * ONE ENTRY (lh264_select_t): list != NULL - the n_list numbers of the list, strictly increasing, none negative (n_list 0: nothing);
 * list == NULL - the range first + k * step for k < count, count 0 meaning "to the stream's end", step >= 1: {NULL, 0, 0, 0, 1} is
 * every picture of the stream.  n_selects is 1 (the entry holds for every stream) or n (one entry per stream).
 * LH264_E_ARG, checked before the device with out untouched, beside every case of the calls above: a struct_bytes other than 24,
 * n_selects other than 0, 1 or n, selects NULL with n_selects > 0, a list that is not strictly increasing or holds a negative number,
 * list NULL with n_list > 0, step 0 in a range, a reserved word that is not 0, a selection together with opts->pick other than
 * LH264_PICK_ALL, a selection together with conceal (for pick's reason, and because deferred records are not concealed). */
typedef struct lh264_select {
  const int32_t* list;                  /* NULL: the range below                                                */
  uint32_t n_list;
  uint32_t first, count, step;          /* list == NULL: first + k * step, k < count (0: to the end), step >= 1  */
} lh264_select_t;
typedef struct lh264_decode_select {
  uint32_t struct_bytes;                /* 24                                                                   */
  uint32_t n_selects;                   /* 0: none (the call is lh264_decode_batch_ex4); 1; or n                */
  const lh264_select_t* selects;
  uint64_t reserved;                    /* 0                                                                    */
} lh264_decode_select_t;
int lh264_decode_batch_ex5 (const uint8_t* const* data, const size_t* len, int n, int threads,
                            const lh264_decode_opts_t* opts /* NULL = defaults */, const lh264_decode_ext_t* ext /* NULL = no colour */,
                            const lh264_decode_sample_t* sample /* NULL = uint8 */, const lh264_decode_view_t* view /* NULL = none */,
                            const lh264_decode_motion_t* motion /* NULL = no fields */, const lh264_decode_select_t* select /* NULL = every picture */,
                            lh264_decoded_t** out);
/* the pictures of the stream that were reconstructed, delivered or not (0 in the motion-only call, which reconstructs nothing) */
long long lh264_decoded_chain_pictures (const lh264_decoded_t* d);
/* the rule above for one Annex-B file and one entry, headers only, no device: the needed pictures and the delivered ones, ascending.
 * The first min (cap_needed, *n_needed) needed numbers go to needed (may be NULL with cap 0), *n_needed is their number whatever the
 * cap is; the same for delivered.  The walk goes no further than the last requested picture and stops where a failure of the header
 * walk stops the call.  LH264_E_ARG: sel NULL or an entry the call above refuses, a count pointer NULL, a cap < 0 */
int lh264_parser_plan (const uint8_t* data, size_t len, const lh264_select_t* sel, int32_t* needed, int cap_needed, int* n_needed,
                       int32_t* delivered, int cap_delivered, int* n_delivered);
/* lh264_decode_batch_ex6: THE FILTER OF A CALL THAT NAMES A SIZE - LH264_FILTER_AREA (the exact area average defined at
 * lh264_decode_batch, the default), LH264_FILTER_BILINEAR (a triangle) or LH264_FILTER_BICUBIC (Catmull-Rom), both widened when
 * shrinking (antialiased), as the resize of an image library is.  The six structs above are frozen; the filter travels in a seventh.
 * filter == NULL or LH264_FILTER_AREA is lh264_decode_batch_ex5, byte for byte and launch for launch (lh264_decode_batch_ex5 is this call
 * with NULL).
 * THE DEFINITION (normative).  One plane of w x h window samples p[y][x] is delivered as ow x oh; a view's source and destination
 * rectangles take the window's and the output's places exactly as for the area average.  Each axis on its own, all arithmetic in
 * integers, `/` is floor.
 *   TAPS of delivered column X (source length w, delivered length ow): m = 2 * max (w, ow); n (x) = |2*ow*x + ow - (2*X + 1)*w|.
 *     n / (2*ow) is the distance from x to the centre (X + 1/2) * w / ow - 1/2, n / m that distance in units of the kernel, which is
 *     widened by w / ow when shrinking.
 *   RAW WEIGHT r (x), for x in 0 .. w - 1 only - nothing outside the window, the crop or the cover rectangle enters; a kernel cut by an
 *     edge is renormalised by what follows.  Bilinear: r = m - n where n < m, else 0.  Bicubic (a = -1/2, times 2 m^3):
 *     n < m: r = 3n^3 - 5n^2 m + 2m^3;  m <= n < 2m: r = -n^3 + 5n^2 m - 8n m^2 + 4m^3;  else 0.
 *   NORMALISED WEIGHT kx (X, x): R = the sum of r over x (> 0: the centre lies inside the window); k = floor ((2^15 * r + R) / (2R))
 *     (for a negative r: toward minus infinity); e = 2^14 - sum k is added to the tap with the largest r, the lowest x among equals.
 *     Every row of weights sums to exactly 2^14.  (r reaches 2^48: the library computes them on the host in 128 bits.)
 *   DELIVERED SAMPLE: ky (Y, y) the same rule with h, oh; H (y, X) = sum_x kx (X, x) * p[y][x] (fits int32);
 *     S = sum_y ky (Y, y) * H (y, X) (int64); sample = clip (0, 255, (S + 2^27) >> 28), the shift arithmetic.  One rounding, at the end.
 *   CHROMA: the same rule on the chroma planes with their own lengths; siting is not modelled, as everywhere in this call.
 * ow == w and oh == h gives the window itself; enlarging, bilinear has two taps a column and one at an edge (edge replication).  The
 * sum of the absolute weights of a row stays far below 2^31 / 255 and every weight fits int16; the table builder checks both and fails
 * the call (LH264_E_HIP on every stream) should either ever be false.  Against a float64 antialiased bilinear / bicubic resize,
 * rounded half up and clipped, the samples differ by at most 1 (informative; the integers above are the definition).
 * The filter applies to stretch, cover, contain and a caller's crop, in I420, NV12, RGB24, planar RGB and the three float types, in
 * every output mode, with digests, pick, select, concealment and both parse routes.  Colour and the float types keep acting on the
 * delivered planes: RGB bytes are the integer function of the I420 bytes the same call delivers without colour, float elements their fma.
 * LH264_E_ARG, checked before the device with out untouched, beside every case of the calls above: a struct_bytes other than 16, a
 * filter above 2, a reserved word that is not 0, a filter other than LH264_FILTER_AREA without out_width / out_height (scale_log2
 * included: it is exclusive with a size). */
#define LH264_FILTER_AREA     0u
#define LH264_FILTER_BILINEAR 1u
#define LH264_FILTER_BICUBIC  2u
typedef struct lh264_decode_filter {
  uint32_t struct_bytes;                /* 16                                                                   */
  uint32_t filter;                      /* LH264_FILTER_*                                                       */
  uint32_t reserved0, reserved1;        /* 0                                                                    */
} lh264_decode_filter_t;
int lh264_decode_batch_ex6 (const uint8_t* const* data, const size_t* len, int n, int threads,
                            const lh264_decode_opts_t* opts /* NULL = defaults */, const lh264_decode_ext_t* ext /* NULL = no colour */,
                            const lh264_decode_sample_t* sample /* NULL = uint8 */, const lh264_decode_view_t* view /* NULL = none */,
                            const lh264_decode_motion_t* motion /* NULL = no fields */, const lh264_decode_select_t* select /* NULL = every picture */,
                            const lh264_decode_filter_t* filter /* NULL = the area average */, lh264_decoded_t** out);
/* the LH264_FILTER_* the call used (LH264_E_ARG: d NULL) */
int lh264_decoded_filter (const lh264_decoded_t* d);
/* the normalised weights of delivered coordinate X of an axis of src_len samples delivered as dst_len, by the definition above, without
 * a device: *first is the first tap's index (the lowest x whose weight is not 0), the first min (cap, *n) weights go to k (may be NULL
 * with cap 0), *n is their number (up to the highest x whose weight is not 0) whatever the cap is.  LH264_E_ARG: LH264_FILTER_AREA
 * (the area average has no such table) or a filter above 2, src_len outside 1..16384, dst_len outside 1..4096, X outside 0..dst_len - 1,
 * first or n NULL, cap < 0, k NULL with cap > 0 */
int lh264_filter_taps (uint32_t filter, int src_len, int dst_len, int X, int32_t* first, int16_t* k, int cap, int* n);
/* one delivered picture's fields to gather (decode_pack_motion_kernel): its mb_w * mb_h records in raster order, its slice table, where
 * the two blocks begin, and back[slot] for every job reference slot (-1: no picture).  The blocks begin at multiples of 8 bytes.
 * lh264_debug_motion_cpu steps the kernel's code over HOST memory with t = 0, nt = 1; lh264_debug_motion_dev uploads the table (its
 * pointers are device pointers), launches the production kernel and returns when it is through.  LH264_E_ARG: jobs NULL, n < 0, a NULL
 * pointer in a job (slices may be NULL with n_slices 0), mb_w or mb_h outside 1..1024, n_slices outside 0..65535, a reserved word that is
 * not 0, a motion or info destination that is not a multiple of 8, and from lh264_debug_motion_dev records that do not begin at a
 * multiple of 16 (the kernel fetches them by 16-byte loads); a bad job anywhere: nothing of the table is done.  lh264_debug_motion_dev
 * without a device: LH264_E_NODEVICE */
typedef struct lh264_motion_job {
  const lh264_mb_t* mbs; const lh264_slice_t* slices;
  int16_t* motion; uint8_t* info;
  int32_t mb_w, mb_h, n_slices, reserved;
  int16_t back[LH264_MAX_REFS];
} lh264_motion_job_t;
#define LH264_MOTION_CHUNK_MBS 64       /* the macroblocks of one macroblock row that a workgroup of the kernel handles */
int lh264_debug_motion_cpu (const lh264_motion_job_t* jobs, int n);
int lh264_debug_motion_dev (const lh264_motion_job_t* jobs, int n);
/* the rule above for a w x h window (even, 2..16384), a crop (NULL or w = h = 0: none), a fit and a size (0, 0: none, stretch only):
 * *src the source rectangle in window coordinates, *dst the destination rectangle in the delivered picture (without a size: {0, 0} and
 * the source's own size).  Either may be NULL.  LH264_E_ARG: a window, crop, fit or size the call above would refuse, a crop that does
 * not fit the window */
int lh264_view_rects (int32_t w, int32_t h, const lh264_rect_t* crop, uint32_t fit, int32_t out_w, int32_t out_h, lh264_rect_t* src, lh264_rect_t* dst);
/* the cropped window of the first SPS of an Annex-B file that parses, without a device: what a caller needs to choose crops before it
 * decodes.  width / height may be NULL.  LH264_E_ARG: data NULL; LH264_E_UNSUPPORTED: no SPS in the file that parses */
int lh264_parser_window (const uint8_t* data, size_t len, int32_t* width, int32_t* height);
/* what the first SPS of an Annex-B file says about colour, without a device: *matrix_coefficients (2 = unspecified where the SPS
 * carries none), *full_range (0 where it carries none), *present bit 0 = the VUI has a video_signal_type, bit 1 = it has a colour
 * description.  Any of the three may be NULL.  LH264_E_ARG: data NULL; LH264_E_UNSUPPORTED: no SPS in the file that parses */
int lh264_parser_colour (const uint8_t* data, size_t len, int32_t* matrix_coefficients, int32_t* full_range, int32_t* present);
int lh264_decoded_status (const lh264_decoded_t* d);
/* how the stream's slice data was parsed: LH264_PARSE_PATH_HOST (none of it on the device), _DEVICE (CAVLC slices by the kernel; CABAC
 * pictures and what follows the first of them by the host - with LH264_PARSE_FLAG_CABAC the slices of both entropy modes by the
 * kernels), _FALLBACK (a slice of some round got a status from a kernel: that round's slices were parsed again by the host and the
 * stream stayed there) */
int lh264_decoded_parse_path (const lh264_decoded_t* d);
/* ... and how many of the stream's slices slice_parse_kernel parsed (a round that fell back, and what the host parsed behind a CABAC
 * picture, do not count; a picture that waited for another round counts once per round it was parsed in) */
long long lh264_decoded_device_slices (const lh264_decoded_t* d);
/* ... and how many of those were CABAC slices, parsed by slice_parse_cabac_kernel (0 without LH264_PARSE_FLAG_CABAC) */
long long lh264_decoded_device_cabac_slices (const lh264_decoded_t* d);
/* the distinct slices of the stream whose slice data was parsed, by the host front end or by a kernel (a slice that waited for another
 * round, or that the host parsed again behind a fallback, counts once): with opts->pick the slices of the selected pictures only,
 * with a selection (lh264_decode_batch_ex5) those of the needed pictures */
long long lh264_decoded_parsed_slices (const lh264_decoded_t* d);
/* the number of delivered picture idx among all pictures the front end found in the stream, in decode order from 0 (withheld and
 * unselected pictures count).  With LH264_PICK_ALL and nothing withheld it equals idx.  LH264_E_ARG: a bad index */
int lh264_decoded_picture_index (const lh264_decoded_t* d, int idx);
const char* lh264_decoded_error (const lh264_decoded_t* d);
int lh264_decoded_pictures (const lh264_decoded_t* d);
int lh264_decoded_picture (const lh264_decoded_t* d, int idx, lh264_decoded_pic_t* out);
/* macroblocks of delivered picture idx that were concealed (0: the picture is what the stream says; < 0: bad argument) */
int lh264_decoded_concealed (const lh264_decoded_t* d, int idx);
/* the cropped window of delivered picture idx before scaling (= its width / height at scale_log2 0); width / height may be NULL.
 * LH264_E_ARG: a bad index */
int lh264_decoded_picture_source_size (const lh264_decoded_t* d, int idx, int32_t* width, int32_t* height);
const uint8_t* lh264_decoded_bytes (const lh264_decoded_t* d, size_t* len);       /* host pointer; NULL in DEVICE_OUT and sink mode */
const uint8_t* lh264_decoded_bytes_dev (const lh264_decoded_t* d, size_t* len);   /* device pointer in DEVICE_OUT mode, else NULL  */
/* DEVICE_OUT mode: the stream's bytes copied into the caller's device memory (cap >= their length), complete on return */
int lh264_decoded_copy_dev (const lh264_decoded_t* d, void* dst_dev, size_t cap);
void lh264_decoded_free (lh264_decoded_t* d);
/* the 20 bytes of a digest the call was asked for.  LH264_E_ARG: a bad index, or a digest that was not asked for; a stream that
 * carries LH264_E_HIP gives that status */
int lh264_decoded_picture_sha1 (const lh264_decoded_t* d, int idx, uint8_t out[20]);
int lh264_decoded_stream_sha1 (const lh264_decoded_t* d, uint8_t out[20]);
int lh264_decode_arena_bytes (size_t* device, size_t* pinned);
void lh264_decode_release (void);
/* milliseconds of the last lh264_decode_batch call in this process: ms[0] the call, ms[1] parsing and picking the rounds' pictures
 * (host threads), ms[2] staging, ms[3] enqueueing the device stage, ms[4] the main thread's wait for the device (the download
 * included), ms[5] delivery (copies into the handles, or the sink).  LH264_TRACE_DECODE=1 prints the same to stderr. */
int lh264_decode_last_timing (double* ms);
/* parse = LH264_PARSE_DEVICE: of ms[1] above, out[0] the milliseconds of the device parse stage (filling tasks, upload, slice_parse_kernel and
 * - with LH264_PARSE_FLAG_CABAC - slice_parse_cabac_kernel, the wait for their results) and out[1] the number of slices it parsed, in the last call (0, 0 under LH264_PARSE_HOST) */
int lh264_decode_last_parse_timing (double* out);
/* the launch shape of the last lh264_decode_batch call in this process: v[0] its rounds (lh264_recon_chains launches), v[1] the chains
 * and v[2] the jobs (pictures) of all of them.  With LH264_PICK_ALL a chain is a stream's pictures of a round; with opts->pick every
 * picture is a chain; with a selection (lh264_decode_batch_ex5) every run of a stream that begins at an IDR picture in the round */
int lh264_decode_last_chains (long long v[3]);
/* the decode-order indices lh264_decode_batch would select from one Annex-B file under `pick` (LH264_PICK_*; LH264_PICK_ALL: every
 * index), up to the first failure of the header walk: the first min (cap, *n) of them go to idx (may be NULL with cap 0), *n is
 * their number whatever cap is.  Headers only, no device is needed.  LH264_E_ARG: a pick that is not defined, n NULL, cap < 0 */
int lh264_parser_pick (const uint8_t* data, size_t len, uint32_t pick, int32_t* idx, int cap, int* n);
/* one picture to crop and pack (decode_pack_kernel): the planes' pixel (0,0) in a padded picture, the window, where the packed
 * picture begins.  crop_x/y/w/h are even.  `reserved` carries the job's scale_log2: 0 = the copy; 1..3 = the means defined at
 * lh264_decode_batch (decode_pack_scaled_kernel), the packed picture then has the delivered size; anything else is LH264_E_ARG.
 * lh264_debug_pack_cpu steps the kernels' code over HOST memory: a check of the crop / format / mean arithmetic where no device is
 * present; not a decode path */
typedef struct lh264_pack_job {
  const uint8_t* y; const uint8_t* u; const uint8_t* v;
  uint8_t* dst;
  int32_t stride_y, stride_c, crop_x, crop_y, crop_w, crop_h, format, reserved;
} lh264_pack_job_t;
int lh264_debug_pack_cpu (const lh264_pack_job_t* jobs, int n);
/* the same jobs on the DEVICE: `jobs` is a host array whose pointers are device pointers.  The table is uploaded, the production kernel
 * for the jobs' scale_log2 (all equal, else LH264_E_ARG) is launched - decode_pack_kernel at 0, decode_pack_scaled_kernel at 1..3 - and
 * the call returns when it is through.  Without a device: LH264_E_NODEVICE.  For tests: windows no stream has */
int lh264_debug_pack_dev (const lh264_pack_job_t* jobs, int n);
/* the same table delivered as out_w x out_h pictures (out_width / out_height at lh264_decode_batch): lh264_debug_resize_cpu steps the
 * code of decode_pack_resized_kernel over HOST memory, lh264_debug_resize_dev uploads the table (its pointers are device pointers),
 * launches the production kernel and returns when it is through.  LH264_E_ARG: a size that is not a pair of even values in 2..4096, a
 * job whose `reserved` is not 0 or whose window is not even, positive and at most 16384 a side, jobs NULL, n <= 0; lh264_debug_resize_dev
 * without a device: LH264_E_NODEVICE */
int lh264_debug_resize_cpu (const lh264_pack_job_t* jobs, int n, int out_w, int out_h);
int lh264_debug_resize_dev (const lh264_pack_job_t* jobs, int n, int out_w, int out_h);
/* the same table delivered as RGB (lh264_decode_batch_ex): layout LH264_COLOUR_RGB24 or LH264_COLOUR_RGBP, std_per_job[k] the standard
 * byte of job k (see LH264_COLOUR_FACTORS; a host array in both calls).  out_w, out_h != 0: every job as out_w x out_h, `reserved` 0;
 * out_w == out_h == 0: each job by its `reserved` scale (0 = the window, 1..3 the means; the jobs of a table may differ).
 * lh264_debug_rgb_cpu steps the code of decode_pack_rgb_kernel over HOST memory, lh264_debug_rgb_dev uploads the two tables (the jobs'
 * pointers are device pointers), launches the production kernel and returns when it is through.  LH264_E_ARG: a layout or a standard
 * byte that is not defined, a size that is neither 0, 0 nor a pair of even values in 2..4096, a `reserved` outside what the size
 * allows, a format other than LH264_FMT_I420, a window that is not even, positive and at most 16384 a side, a NULL table, n <= 0;
 * lh264_debug_rgb_dev without a device: LH264_E_NODEVICE */
int lh264_debug_rgb_cpu (const lh264_pack_job_t* jobs, int n, int out_w, int out_h, int layout, const uint8_t* std_per_job);
int lh264_debug_rgb_dev (const lh264_pack_job_t* jobs, int n, int out_w, int out_h, int layout, const uint8_t* std_per_job);
/* the same table delivered as float RGB (lh264_decode_batch_ex2): the arguments above and the sample struct, which must name a float
 * type.  lh264_debug_sample_cpu steps the code of decode_pack_sample_kernel over HOST memory with t = 0, nt = 1, lh264_debug_sample_dev
 * uploads the two tables, launches the production kernel and returns when it is through.  LH264_E_ARG: everything the RGB entry points
 * refuse, a sample struct lh264_decode_batch_ex2 refuses or whose type is LH264_SAMPLE_U8 or that is NULL, a job whose dst is not a
 * multiple of 4; lh264_debug_sample_dev without a device: LH264_E_NODEVICE */
int lh264_debug_sample_cpu (const lh264_pack_job_t* jobs, int n, int out_w, int out_h, int layout, const uint8_t* std_per_job, const lh264_decode_sample_t* sample);
int lh264_debug_sample_dev (const lh264_pack_job_t* jobs, int n, int out_w, int out_h, int layout, const uint8_t* std_per_job, const lh264_decode_sample_t* sample);
/* the host stepping's conversions of n binary32 values to 16 bits (type LH264_SAMPLE_F16 or _BF16, anything else LH264_E_ARG): what
 * lh264_debug_sample_cpu rounds with, laid open so that a test can show it is nearest even at every boundary.  No device is needed */
int lh264_debug_sample_round (uint32_t type, const float* v, size_t n, uint16_t* out);
/* where a job's picture is placed in an out_w x out_h picture (LH264_FIT_CONTAIN): the window is resampled to w x h at (x, y), every
 * sample outside that rectangle is the fill (fill_y | fill_cb << 8 | fill_cr << 16).  x, y, w, h are even, w, h >= 2, the rectangle
 * lies inside the delivered picture; `reserved` is 0.  The kernels read one record per pack job from a table beside the jobs' */
typedef struct lh264_pack_place { int32_t x, y, w, h; uint32_t fill, reserved; } lh264_pack_place_t;
/* the same table delivered as out_w x out_h pictures with job k placed by places[k]: colour == 0 the planes in each job's format
 * (decode_pack_placed_kernel), colour LH264_COLOUR_RGB24 / _RGBP RGB bytes (decode_pack_rgb_placed_kernel; std_per_job as above, may be
 * NULL with colour 0), and with a sample struct that names a float type float RGB (decode_pack_sample_placed_kernel; sample NULL or
 * LH264_SAMPLE_U8: bytes).  lh264_debug_view_cpu steps the kernels' code over HOST memory with t = 0, nt = 1, lh264_debug_view_dev
 * uploads the tables (the jobs' pointers are device pointers), launches the production kernel and returns when it is through.
 * LH264_E_ARG: everything the sibling for that path refuses (out_w, out_h are a size here, never 0, 0), places NULL, a place rectangle
 * that is odd, below 2 x 2 or outside out_w x out_h, a fill above 24 bits, a place whose `reserved` is not 0; lh264_debug_view_dev
 * without a device: LH264_E_NODEVICE */
int lh264_debug_view_cpu (const lh264_pack_job_t* jobs, const lh264_pack_place_t* places, int n, int out_w, int out_h, int colour, const uint8_t* std_per_job, const lh264_decode_sample_t* sample);
int lh264_debug_view_dev (const lh264_pack_job_t* jobs, const lh264_pack_place_t* places, int n, int out_w, int out_h, int colour, const uint8_t* std_per_job, const lh264_decode_sample_t* sample);
/* the same table delivered as out_w x out_h pictures resampled by `filter` (LH264_FILTER_BILINEAR or _BICUBIC, lh264_decode_batch_ex6):
 * places NULL - every window to the whole picture - or job k placed by places[k]; colour, std_per_job and sample as above
 * (decode_pack_filtered_kernel, decode_pack_rgb_filtered_kernel, decode_pack_sample_filtered_kernel).  The weight tables of the jobs'
 * geometries are built by the call.  lh264_debug_filter_cpu steps the kernels' code over HOST memory with t = 0, nt = 1,
 * lh264_debug_filter_dev uploads the tables (the jobs' pointers are device pointers), launches the production kernel and returns when
 * it is through.  LH264_E_ARG: everything lh264_debug_view_cpu refuses (but places may be NULL), a filter that is not 1 or 2;
 * lh264_debug_filter_dev without a device: LH264_E_NODEVICE */
int lh264_debug_filter_cpu (const lh264_pack_job_t* jobs, const lh264_pack_place_t* places, int n, int out_w, int out_h, uint32_t filter, int colour, const uint8_t* std_per_job, const lh264_decode_sample_t* sample);
int lh264_debug_filter_dev (const lh264_pack_job_t* jobs, const lh264_pack_place_t* places, int n, int out_w, int out_h, uint32_t filter, int colour, const uint8_t* std_per_job, const lh264_decode_sample_t* sample);
/* SHA-1 of n_messages messages given as spans of `bytes`: n_spans triples {message, offset, length}, in order.  The k-th span of
 * every message is fed in step k - on the device (on_device != 0) one launch of sha1_spans_kernel per step, the state carried from
 * step to step as a stream's is from round to round; on_device = 0 steps the same code on the host and needs no device.  A message
 * without a span is the empty message.  out: 20 bytes per message */
int lh264_debug_sha1 (const uint8_t* bytes, const uint64_t* spans, int n_spans, int n_messages, int on_device, uint8_t* out);
/* The CAVLC macroblock layer apart from the header walk (csrc/lh264_slice.h, slice_parse_kernel): one Annex-B stream goes through the
 * deferred parser (lh264_parser_set_defer_slice_data), then every deferred slice through the one piece of code that parses slice data
 * for the device - stepped on `threads` host threads (on_device = 0, needs no device) or run by slice_parse_kernel, one wave per slice
 * (on_device != 0; LH264_E_NODEVICE without one).  The handle gives per picture what that code wrote: the records, the dense
 * coefficient plane (768 bytes per macroblock), the slice table with n_mbs, and per slice 4 x int32 {1 = the slice was deferred, status,
 * n_mbs, the bit position behind the last macroblock}; status 0 = parsed as the host front end parses it, 1 = syntax the host front end
 * fails on, 2 = the slice would run into the next slice's first macroblock (nothing at or beyond it is written), 3 = an inconsistent
 * task.  Every buffer the code reads or writes lies in one arena with 64 guard bytes behind it; lh264_slice_dump_guards_ok: 1 when all
 * of them are intact after the run.  tweak (may be NULL): {picture, slice, limit_mb} replaces the limit of one slice - the macroblock
 * at which it must stop - for tests of the overrun status.  lh264_slice_dump_error: the header walk's error text.  Not a decode path.
 * lh264_debug_slice_parse_opts is the same call with flags: LH264_SLICE_PARSE_ON_DEVICE for on_device, and LH264_SLICE_PARSE_CABAC, with
 * which CABAC slices are deferred too (lh264_parser_set_defer_cabac) and walked by csrc/lh264_slice_cabac.h, on the host threads or by
 * slice_parse_cabac_kernel; the bit position of such a slice is the arithmetic decoder's.  Without that flag a CABAC stream defers
 * nothing, as with lh264_debug_slice_parse, which forwards here.  Its tweak has a fourth entry: >= 0 replaces the byte of the slice's
 * task that names the entropy mode and cabac_init_idc (0 = CAVLC, 0x80 | idc = CABAC), for tests of the inconsistent-task status */
typedef struct lh264_slice_dump lh264_slice_dump_t;
#define LH264_SLICE_PARSE_ON_DEVICE 1u
#define LH264_SLICE_PARSE_CABAC     2u
int lh264_debug_slice_parse (const uint8_t* data, size_t len, int on_device, int threads, const int32_t* tweak, lh264_slice_dump_t** out);
int lh264_debug_slice_parse_opts (const uint8_t* data, size_t len, uint32_t flags, int threads, const int32_t* tweak /* [4] */, lh264_slice_dump_t** out);
int lh264_slice_dump_pictures (const lh264_slice_dump_t* d);
int lh264_slice_dump_picture (const lh264_slice_dump_t* d, int idx, int32_t info[4] /* mb_w, mb_h, slices, deferred slices */);
const lh264_mb_t* lh264_slice_dump_mbs (const lh264_slice_dump_t* d, int idx);
const int16_t* lh264_slice_dump_coeffs (const lh264_slice_dump_t* d, int idx);
const lh264_slice_t* lh264_slice_dump_slices (const lh264_slice_dump_t* d, int idx);
const int32_t* lh264_slice_dump_results (const lh264_slice_dump_t* d, int idx);
int lh264_slice_dump_guards_ok (const lh264_slice_dump_t* d);
const char* lh264_slice_dump_error (const lh264_slice_dump_t* d);
void lh264_slice_dump_free (lh264_slice_dump_t* d);
/* the launch geometry lh264_recon_chains / lh264_recon_frames would choose for pictures of at most max_mb_w x max_mb_h macroblocks:
 * waves per workgroup (one per macroblock row in flight, at most 8, halved until the LDS line buffers fit; LH264_WAVES is honoured as
 * in a launch) and the dynamic LDS bytes.  Read-only, needs no device.  LH264_E_UNSUPPORTED with the launch's own text when one wave
 * does not fit (the outputs are still written: 1 wave and the bytes it would need); LH264_E_ARG: a dimension <= 0 */
int lh264_debug_recon_geometry (int max_mb_w, int max_mb_h, int* waves, size_t* lds_bytes);

#define LH264_OK            0
#define LH264_E_NODEVICE   -1
#define LH264_E_ARG        -2
#define LH264_E_HIP        -3
#define LH264_E_UNSUPPORTED -4

#ifdef __cplusplus
}
#endif
#endif /* LH264_H_ */
