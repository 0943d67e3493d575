/* v2x_amd.h -- C ABI of libv2x_amd.so: the MI355X (gfx950) hot path of the V2X-Sim
 * collaborative-perception baselines.
 *
 * What each entry point replaces.  The reference checkout holds no code: the
 * whole path lives in the un-vendored submodule `coperception`
 * (/root/reference/.gitmodules:1-3; /root/reference/README.md:101 names the
 * det/seg benchmarks, README.md:45 the create_data.py voxelisation).  The
 * reference has no FFI/plugin interface of its own -- its "operator API" is
 * torch.nn.Module.forward -- so every entry below cites the upstream python
 * function (path only; no line numbers exist in the tree) whose arithmetic it
 * takes over.  INTEGRATION.md shows the ctypes stub a maintainer would add.
 *
 * Conventions: plain pointers and sizes only (no torch types); all pointers are
 * DEVICE pointers unless marked host; the caller owns every buffer (no internal
 * allocation, no global mutable state); `stream` is a hipStream_t passed as
 * void*; calls are asynchronous on that stream and re-entrant; the return value
 * is 0 or a negative errno-style code, and v2x_last_error() gives the text for
 * the calling thread.  bf16 tensors are passed as uint16_t*.
 *
 * Tensor layouts: activations are NHWC ("BEV pixel major, channels fastest"),
 * which is the reference's own (X, Y, Z) voxel-grid layout with Z as channels.
 */
#ifndef V2X_AMD_H
#define V2X_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define V2X_AMD_ABI_VERSION 18

#define V2X_OK 0
#define V2X_EINVAL (-22) /* bad argument / unsupported shape */
#define V2X_EIO (-5)     /* HIP launch failure */

typedef void *v2x_stream_t; /* hipStream_t */

/* V2X_AMD_ABI_VERSION of the library; NEGATIVE (-V2X_AMD_ABI_VERSION) when the library contains an instrumented kernel object (a tools/probes/ timing build:
 * phase-removal switches, time stamps -- its results are garbage): a caller that checks the version, as every caller should, then refuses it. */
int v2x_abi_version(void);
const char *v2x_last_error(void);

/* Kernel-selection switches.  The library picks, per layer shape, the kernel form that measured fastest; a few shapes have a second
 * form that computes the same result (the bitwise-equality tests and the paired A/B tool compare them).  `name` is one of
 *   STREAM_WAVES (8 | 4)  STREAM_G  STREAM_WT (0 | 1 | 2)  STORE_X4  STREAM_PERSIST  STREAM_WIDE  WIDE3  HALO_PP  S2_G
 *   VOXELIZE_LDS (0 | 1 | 2)  WARP_LDS  GRU_XCD_WALK  HALO_XCD  WGRAD_TR  BN_PARTIAL_T  WGRAD_REDUCE4  CONV1X1     (0 | 1 unless noted; case-insensitive, an optional "V2X_" prefix is ignored)
 * Each switch is initialised ONCE, at first use, from the environment variable V2X_<NAME> when that is set; afterwards only
 * v2x_tuning_set changes it (process-wide, relaxed atomics: set it before the launches it should affect).  No upstream
 * counterpart (the reference has one implementation per operator).  Unknown name -> V2X_EINVAL. */
int v2x_tuning_set(const char *name, int value);
int v2x_tuning_get(const char *name, int *value);

/* ---------------------------------------------------------------- a1: voxel scatter
 * Replaces coperception/utils/data_util.py::voxelize_occupy (range filter,
 * floor(p / voxel) in fp64, dedupe, dense occupancy) and the densify scatter of
 * coperception/datasets/V2XSimDet.py::__getitem__.
 *
 * pts:   [n_clouds][max_pts][pt_stride] fp32, x,y,z first; cloud i holds n_pts[i] points.
 * extents {xlo,xhi,ylo,yhi,zlo,zhi}, voxel {vx,vy,vz}: HOST fp64 arrays.
 * bits:  [n_clouds][X][Y] uint32, bit z set iff voxel (x,y,z) is occupied (Z <= 32).
 *        The call clears `bits` itself (memset node on `stream`) before scattering. */
int v2x_voxelize_bits(const float *pts, const int32_t *n_pts, int n_clouds, int max_pts, int pt_stride,
                      const double *extents, const double *voxel, const int32_t *dims_xyz,
                      uint32_t *bits, v2x_stream_t stream);

/* Early fusion (the "upperbound" baseline, README.md:101): upstream merges the clouds of all agents into the
 * ego frame at data-preparation time (create_data_det.py, CPU) and voxelizes the union.  Here job j moves source
 * cloud src_cloud[j] by the rigid transform xform[j] (device fp32 [n_jobs][3][4], row-major) and scatters it into
 * target grid dst_grid[j]; several jobs may share a target.  fp32 transform with separately rounded ops in the
 * order ((x*m0 + y*m1) + z*m2) + m3, then the a1 index spec.  bits: [n_grids][X][Y], cleared by the call. */
int v2x_voxelize_fused_bits(const float *pts, const int32_t *n_pts, int n_clouds, int max_pts, int pt_stride,
                            const float *xform, const int32_t *src_cloud, const int32_t *dst_grid, int n_jobs,
                            int n_grids, const double *extents, const double *voxel, const int32_t *dims_xyz,
                            uint32_t *bits, v2x_stream_t stream);

/* bits -> the reference's dense padded_voxel_points layout [n][X][Y][Z] fp32 {0,1}. */
int v2x_bits_to_dense_f32(const uint32_t *bits, int n, int X, int Y, int Z, float *out, v2x_stream_t stream);

/* bits -> network input: NHWC bf16 [n][X][Y][c_pad], channels >= Z are zero. c_pad % 8 == 0. */
int v2x_bits_to_nhwc_bf16(const uint32_t *bits, int n, int X, int Y, int Z, int c_pad, uint16_t *out,
                          v2x_stream_t stream);

/* dense fp32 bevs [n][X][Y][Z] (what the reference Dataset hands the model) -> NHWC bf16 [n][X][Y][c_pad]. */
int v2x_dense_f32_to_nhwc_bf16(const float *bev, int n, int X, int Y, int Z, int c_pad, uint16_t *out,
                               v2x_stream_t stream);

/* bits -> sorted (x,y,z)-lexicographic voxel indices, as voxelize_occupy(return_indices=True).
 * idx: [n][cap][3] int32; counts: [n] int32 (true count even if > cap; only `cap` are written).
 * scratch: [n][X] int32 device workspace. */
int v2x_bits_to_indices(const uint32_t *bits, int n, int X, int Y, int Z, int32_t *idx, int cap, int32_t *counts,
                        int32_t *scratch, v2x_stream_t stream);

/* Densify: the parsed dataset stores each sweep as sparse voxel indices (README.md:66-79 layout;
 * upstream V2XSimDet.__getitem__: curr_voxels[idx[:,0], idx[:,1], idx[:,2]] = 1).  idx: [n][cap][3] int32,
 * counts: [n]; bits as v2x_voxelize_bits (cleared by the call). */
int v2x_indices_to_bits(const int32_t *idx, const int32_t *counts, int n, int cap, int X, int Y, int Z,
                        uint32_t *bits, v2x_stream_t stream);

/* ---------------------------------------------------------------- a2/a4/a6/a7/a8: convolutions
 * One implicit-GEMM MFMA kernel family covers
 *   - coperception/models/det/backbone/Backbone.py::LidarEncoder / LidarDecoder
 *     (3x3 stride 1/2 conv + BN + ReLU; the 1x1x1 "Conv3D"; F.interpolate(x2) +
 *      torch.cat + conv fused through the two-source loader),
 *   - convolutional_rnn.Conv2dGRU one cell step with h0 = 0 (V2VNet.py), gates
 *     fused in the epilogue,
 *   - DetModelBase.py::ClassificationHead / SingleRegressionHead and the seg head,
 *   - When2com.py::PolicyNet4 convs and KmGenerator linears (as 1x1 convs on 1x1 maps).
 */
enum {
    V2X_EPI_BF16 = 0, /* y = acc*scale[c] + shift[c], optional ReLU, bf16 NHWC out          */
    V2X_EPI_F32 = 1,  /* same, fp32 NHWC out (logits)                                        */
    V2X_EPI_GRU = 2,  /* rows are (r,z,n) gate triples; out = (1-z)*n, bf16; see DESIGN.md   */
    V2X_EPI_DET = 3   /* detection heads with the score threshold fused in (halo kernel, chained layer only): instead of the
                       * logits the launch emits the candidates of upstream postprocess.py::apply_nms_det's first step,
                       * softmax(cls)[1] >= det_thr, ready for v2x_det_nms_candidates.  Shape: 3x3 32 -> 64 hidden (cls | reg,
                       * chain order) chained with Cout2 = 64 rows in DET ORDER: packed row 16 t + 4 q + r, q < 3, belongs to
                       * the anchors a0 = 2 q, a1 = 2 q + 1 of the pixel:  t = 0: cls[a0][0], cls[a0][1], cls[a1][0], cls[a1][1];
                       * t = 1: loc[a0][0..3];  t = 2: loc[a0][4], loc[a0][5], loc[a1][0], loc[a1][1];  t = 3: loc[a1][2..5];
                       * rows with q = 3 are zero (6 anchors x (2 + 6) = 48 real rows of 64).  out = keys uint64
                       * [N][det_cap] (~score bits << 32 | anchor index << 12 | slot), out2 = codes fp32 [N][det_cap][6],
                       * det_counts int32 [N] (ZEROED BY THE CALLER; the true count even when > det_cap).  H*W*6 < 2^20. */
};

typedef struct v2x_conv_desc {
    const uint16_t *in0; /* bf16 NHWC [N][H>>up0][W>>up0][C0]                                     */
    const uint16_t *in1; /* bf16 NHWC [N][H][W][C1] or NULL; logical input = cat(up(in0), in1)   */
    int32_t C0, C1;      /* C0 % 8 == 0, C1 % 8 == 0                                              */
    int32_t up0;         /* log2 nearest-neighbour upsample applied to in0 (0 or 1)              */
    int32_t N, H, W;     /* logical input extent                                                 */
    int32_t ksize;       /* 1 or 3                                                               */
    int32_t stride;      /* 1 or 2                                                               */
    int32_t pad;         /* 0 or 1                                                               */
    int32_t Cout;        /* logical output channels (GRU: hidden channels)                       */
    int32_t w_rows;      /* packed weight rows (multiple of v2x_conv_tile_rows)                  */
    int32_t w_kpad;      /* packed K extent, multiple of 64, >= ksize*ksize*(C0+C1)              */
    const uint16_t *weight; /* bf16 [w_rows][w_kpad], k = (ky*ksize+kx)*(C0+C1) + c              */
    const float *scale;  /* fp32 [w_rows]   (GRU: float4 [Cout] = b_ir+b_hr, b_iz+b_hz, b_in, b_hn) */
    const float *shift;  /* fp32 [w_rows]   (GRU: unused)                                        */
    int32_t epilogue;    /* V2X_EPI_*                                                            */
    int32_t relu;
    void *out;           /* NHWC [N][Ho][Wo][out_cstride], written at channel offset out_coff    */
    int32_t out_cstride, out_coff;
    void *out2;          /* optional second NHWC output: channels >= split go to out2[..][c-split] */
    int32_t split;       /* multiple of 4; 0 = no split (out2 ignored)                           */
    int32_t out2_cstride;
    /* --- halo-tile kernel (conv_halo.hip): 3x3 stride-1 layers with <= 96 input channels ------ */
    int32_t w_layout;    /* 4: the same for the STREAMED layers (conv_stream_pc.hip: conv5_1, conv6_1; Cout % 128 == 0, H % 16 == 0,    */
                         /*    W % 32 == 0); w_kpad = 16*C0 + 9*C1                                                                */
                         /* 3: parity-class form of a decoder layer cat(up(in0), in1) -> 3x3 (conv_halo.hip, conv8_1's shape   */
                         /*    C0 = 64, C1 = 32, Cout = 32; H%8==0, W%32==0): see "weight layouts"; w_kpad = 16*C0 + 9*C1     */
                         /* 0: row-major [w_rows][w_kpad] (gather kernel)                          */
                         /* 1: k-slot-major [9*Cin/8][Cout][8] (halo kernel; H%8==0, W%32==0)      */
                         /* 2: streamed slices [co_tile][Cin/32][9][4][rows][8] (conv_stream.hip:    */
                         /*    3x3 stride 1, C0,C1 % 32 == 0, tiles 8x32 / 16x32 / 16x16;           */
                         /*    conv_stream_s2.hip: 3x3 stride 2, one source, H % 8 == 0, W % 64 == 0) */
    int32_t Cout2;       /* > 0: chain a 1x1 conv on the (never stored) Cout-channel result:       */
    const uint16_t *weight2; /* bf16 [ceil16(Cout2)][Cout] row-major; `epilogue`/`split`/out* then  */
    const float *scale2; /*   describe the FINAL output, scale/shift/relu the hidden layer and     */
    const float *shift2; /*   scale2/shift2/relu2 (fp32 [ceil16(Cout2)]) the chained one.          */
    int32_t relu2;       /*   weight rows must be in the chain order ("weight layouts" below).     */
    int32_t in_format;   /* 0: in0 is bf16 NHWC.  1 (w_layout 1, C0 == 32, C1 == 0 only): in0 is the voxelizer's  */
    int32_t in_zbits;    /*    uint32 bit grid [N][H][W]; bit z < in_zbits = channel z, expanded on the fly.      */
    int32_t *det_counts; /* V2X_EPI_DET only (else NULL / 0): candidate counters [N], score threshold, slots per map   */
    float det_thr;
    int32_t det_cap;     /*    <= 4096                                                                              */
    int32_t splitk;      /* > 1 (w_layout 2, stride 1 or 2, no chained layer): small-batch form -- the 32-channel chunks are divided */
    float *splitk_ws;    /*    into `splitk` contiguous ranges computed by different workgroups; fp32 workspace                   */
                         /*    [splitk][N*Ho*Wo][w_rows] (output pixels), caller-owned.  The partial sums are added in range order (deterministic;  */
                         /*    fp32 summation order differs from the unsplit kernels: one bf16 rounding of the output).  Needs    */
                         /*    splitk <= (C0 + C1) / 32 with no empty range: ceil(chunks / splitk) * (splitk - 1) < chunks.        */
    int32_t small_batch; /* 0 (default): the kernel form follows the layer SHAPE only, never N -- a rank that owns fewer items launches the    */
                         /*    same kernels and produces the same bits (R-rank == 1-rank).  1: the CALLER declares a latency launch: forms    */
                         /*    whose choice depends on the tile count may be taken (stride-2 layers: the 1-tap 128-pixel kernel instead of    */
                         /*    the 8-wave three-tap one below 4 tiles per CU; fp32 summation order differs between the two).                 */
} v2x_conv_desc;

/* ---------------------------------------------------------------- weight layouts and their packers (HOST side)
 * A checkpoint holds conv weights as fp32 OIHW [Cout][Cin][k][k] (the ConvGRU: weight_ih [3*hidden][Cin][3][3], gates in
 * (r, z, n) order).  Every kernel reads bf16 (round-to-nearest-even) in one of five layouts, selected by
 * v2x_conv_desc.w_layout.  With Cin' = Cin zero-padded to `cin_pad`, K = k*k*Cin' and the reduction index
 * kk = (ky*k + kx)*Cin' + c  (tap-major, channels fastest, matching NHWC activations):
 *
 *   w_layout 0 (gather kernel, any shape):  [w_rows][w_kpad] row-major; w_rows = Cout rounded up to
 *       v2x_conv_tile_rows(Cout, epilogue), w_kpad = K rounded up to 64, padding = zeros.  scale / shift hold w_rows floats.
 *       GRU: w_rows = hidden/16*48; packed row g*48 + gate*16 + e holds source row gate*hidden + g*16 + e, i.e. the
 *       (r, z, n) rows of 16 hidden channels are adjacent so that one wave owns all three gates of its channels; `scale`
 *       is then float4 [hidden] = (b_ir + b_hr, b_iz + b_hz, b_in, b_hn)  (v2x_pack_gru_bias), `shift` unused.
 *   w_layout 1 (halo kernel, 3x3 stride 1, Cin' % 32 == 0, Cout % 32 == 0):  k-slot-major [K/8][Cout][8]: element
 *       (s, co, j) = W[co][kk = 8*s + j].  w_rows = Cout, w_kpad = K; scale / shift hold Cout floats in natural order.
 *   w_layout 2 (streamed kernels, 3x3, Cin' % 32 == 0, Cout % 64 == 0 or GRU hidden % 32 == 0):  slices
 *       [co_tile][Cin'/32][9 taps][4 slots][rows][8] with rows = v2x_conv_stream_tile_rows(Cout, epilogue): element
 *       (t, ch, tap, slot, r, j) = W[t*rows + r][kk = tap*Cin' + 32*ch + 8*slot + j], followed by 64 B of zeros (the
 *       kernel's zero page).  GRU rows in the (r, z, n)-triple order above (w_rows = 3*hidden); w_kpad = K.
 *   w_layout 3 (parity-class halo kernel; decoder layers F.interpolate(x, 2) + torch.cat + 3x3 of Backbone.py::LidarDecoder, Cin = c_up + C1):
 *       for an output pixel (2Y + py, 2X + px) the three tap rows of the 3x3 read only TWO rows of the half-resolution source -- ky in
 *       G(py, a), a = 0, 1, with G(0,0) = {0}, G(0,1) = {1,2}, G(1,0) = {0,1}, G(1,1) = {2} -- and likewise the columns, so per parity class
 *       (py, px) the upsampled half of the layer is a 2x2-tap convolution on the half-resolution map with the weights
 *       W'[py][px][a][b][co][c] = sum over ky in G(py,a), kx in G(px,b) of W[co][c][ky][kx]  (c < c_up), added in fp32 in (ky, kx) ascending
 *       order and rounded to bf16 ONCE: 4 c_up + 9 C1 instead of 9 (c_up + C1) multiply-adds per output.  Buffer:
 *       [class 2*py+px][tap 2*a+b][c_up/8][Cout][8] followed by the skip half [tap 3*ky+kx][C1/8][Cout][8];  w_rows = Cout,
 *       w_kpad = 16*c_up + 9*C1.  (No upstream counterpart: an exact identity in real arithmetic; the tests hold the kernel to the
 *       unmodified fp32 9-tap layer at the tolerance of the 9-tap kernel.)
 *   w_layout 4 (streamed parity-class kernel; the same identity for Cout % 128 == 0): per 128-row channel tile
 *       [c_up/32 chunks][class tap 2*a+b][class 2*py+px][4 k-slots][128 rows][8] with the pre-summed weights of layout 3, then
 *       [C1/32 chunks][kx][ky][4 k-slots][128 rows][8]; after the last tile 64 B of zeros (the kernel's zero page).  w_rows = Cout,
 *       w_kpad = 16*c_up + 9*C1.
 *   chained layers (Cout2 > 0; layouts 1 and 2): the rows of the FIRST layer are stored in "chain order": packed row
 *       rho = 16*i + 4*q + r holds output channel kappa = 32*(i>>1) + 8*q + 4*(i&1) + r (a lane's accumulators of the first
 *       GEMM are then exactly its B fragment of the second); its scale / shift stay in natural channel order.  The chained
 *       1x1 weights are bf16 [ceil16(Cout2)][Cout] row-major, scale2 / shift2 fp32 [ceil16(Cout2)]  (v2x_pack_chain_1x1).
 *
 * The packers below run on the HOST (no GPU call): query the size, allocate, pack, upload, fill the descriptor. */
typedef struct v2x_pack_spec {
    int32_t Cout;     /* output channels (GRU: hidden channels; the source tensor then has 3*Cout rows) */
    int32_t Cin;      /* input channels of the source tensor                                             */
    int32_t ksize;    /* 1 or 3                                                                          */
    int32_t cin_pad;  /* 0 = Cin, else Cin zero-padded to this many channels (13 -> 32 for the first layer); % 8 == 0 */
    int32_t w_layout; /* 0, 1 or 2 (above)                                                               */
    int32_t epilogue; /* V2X_EPI_*: selects the row tile; V2X_EPI_GRU = (r, z, n) row regrouping           */
    int32_t chain;    /* 1: the layer is followed by a chained 1x1 (Cout2 > 0): rows in chain order       */
    int32_t c_up;     /* w_layout 3 and 4 only: the first c_up input channels are the x2-upsampled source (v2x_conv_desc.C0); else 0 */
    /* ABI 17, v2x_pack_conv_device / _job with transform = 1 only (0, 0 everywhere else): the data-gradient layer of a SLICE of a convolution's input
     * channels -- rows src_row0 .. src_row0 + Cout - 1 of the src_rows rows the full data-gradient layer has (src_rows = the convolution's Cin; the
     * weights are read from its whole tensor W [Cin = this spec's][src_rows][k][k]).  Lets a data gradient be computed as several launches that each
     * fit a kernel (conv8_1 of the decoder: 32 -> 96 channels as 32 -> 64 and 32 -> 32 into one 96-channel map). */
    int32_t src_rows, src_row0;
} v2x_pack_spec;

/* Bytes of the packed bf16 buffer (0 = unsupported spec, see v2x_last_error) and the w_rows / w_kpad to put in the descriptor. */
size_t v2x_pack_conv_size(const v2x_pack_spec *spec, int32_t *w_rows, int32_t *w_kpad);
/* w_oihw: HOST fp32 [rows][Cin][k][k]; dst: HOST buffer of v2x_pack_conv_size bytes. */
int v2x_pack_conv(const v2x_pack_spec *spec, const float *w_oihw, uint16_t *dst);
/* The same packing as v2x_pack_conv ON THE DEVICE, one launch (training re-packs every layer after every optimizer step): w_oihw_dev
 * fp32 DEVICE [rows][Cin][k][k], dst_dev DEVICE buffer of v2x_pack_conv_size bytes, bit-identical to the host packer's output.
 * transform = 1: `spec` describes the DATA-GRADIENT layer of a convolution (spec->Cout = its Cin, spec->Cin = its Cout) and the weights
 * W'[o][c][ky][kx] = W[c][o][2-ky][2-kx] are read from the convolution's own tensor W [spec->Cin][spec->Cout][k][k].  Plain layers only
 * (no V2X_EPI_GRU regrouping, chain = 0). */
int v2x_pack_conv_device(const v2x_pack_spec *spec, const float *w_oihw_dev, int transform, uint16_t *dst_dev, v2x_stream_t stream);
/* Many layers in ONE launch (a training step re-packs ~55 layers after its optimizer step; one launch each was 0.23 ms of a 6-ms step on the
 * launch floor).  v2x_pack_conv_device_job fills ONE job on the HOST for the packing v2x_pack_conv_device would do -- same arguments;
 * block_begin = the sum of the n_blocks of the jobs in front of it -- and returns its block count in *n_blocks.  The caller copies the job array
 * to the device once (jobs hold device pointers: valid while the parameters and destination buffers stay where they are) and calls
 * v2x_pack_conv_device_batch(jobs_dev, n_jobs, total_blocks) after every update.  Bit-identical to the per-layer launches. */
typedef struct v2x_pack_job {
    const float *w;       /* DEVICE fp32 parameter            */
    uint16_t *dst;        /* DEVICE packed bf16 destination   */
    int32_t rows_src, cin, cin_p, taps, K, w_kpad, tile, cout, layout, transform;
    int32_t src_stride, reserved0; /* transform = 1: rows of the source tensor per input channel (= rows_src unless the job packs a row slice)  */
    int64_t groups, data_groups;   /* 16-byte groups of the destination; of them real rows */
    int64_t block_begin;  /* first workgroup of this job in the batched launch */
} v2x_pack_job;
int v2x_pack_conv_device_job(const v2x_pack_spec *spec, const float *w_oihw_dev, int transform, uint16_t *dst_dev, int64_t block_begin,
                             v2x_pack_job *job_host, int64_t *n_blocks);
int v2x_pack_conv_device_batch(const v2x_pack_job *jobs_dev, int32_t n_jobs, int64_t total_blocks, v2x_stream_t stream);
/* Chained 1x1: w2 HOST fp32 [Cout2][Cout] -> dst_w bf16 [ceil16(Cout2)][Cout]; scale2 / shift2 (NULL = ones / zeros)
 * -> fp32 [ceil16(Cout2)], zero beyond Cout2. */
int v2x_pack_chain_1x1(int Cout2, int Cout, const float *w2, const float *scale2, const float *shift2, uint16_t *dst_w,
                       float *dst_scale, float *dst_shift);
/* ConvGRU biases (h0 = 0): bias_ih, bias_hh HOST fp32 [3*hidden] -> dst float4 [hidden] = (b_ir+b_hr, b_iz+b_hz, b_in, b_hn). */
int v2x_pack_gru_bias(int hidden, const float *bias_ih, const float *bias_hh, float *dst);
/* Eval-mode BatchNorm folded behind the fp32 accumulation: scale = gamma / sqrt(var + eps), shift = beta + scale*(conv_bias
 * - mean); gamma == NULL: no BN (scale 1, shift = conv_bias).  Writes n_out >= C floats each, zeros beyond C. */
int v2x_fold_bn(int C, int n_out, const float *conv_bias, const float *gamma, const float *beta, const float *mean,
                const float *var, float eps, float *scale, float *shift);

/* Rows-per-tile the kernel will use for (Cout, epilogue); the weight packer pads w_rows to a multiple. */
int v2x_conv_tile_rows(int Cout, int epilogue);
/* Same for the streamed-weights kernel (w_layout 2); 0 = that kernel does not cover (Cout, epilogue). */
int v2x_conv_stream_tile_rows(int Cout, int epilogue);
int v2x_conv2d(const v2x_conv_desc *desc, v2x_stream_t stream);
/* The kernel(s) v2x_conv2d(desc) WOULD launch, from the code path that launches them: the same validation and dispatch run with the launch itself
 * replaced by a record of the kernel's own symbol name.  buf receives the names as a profiler prints them (template arguments, no argument list:
 * "conv3x3_stream8g_kernel<96, 2, false>"), a sequence (split-K: partial sums, then the reduce) joined with " + ", NUL-terminated.  Returns what
 * v2x_conv2d returns for this descriptor (same codes, same v2x_last_error text), V2X_EINVAL if the names do not fit cap bytes.  Nothing is
 * launched, no tensor pointer is dereferenced and no GPU is needed: without one the dispatch rules that count CUs assume the MI355X's 256 (with
 * one, the CU count is read as in a launch: hipGetDevice / hipDeviceGetAttribute, the only HIP calls).  The pointers still count: they must be
 * non-null, and the 1x1 streaming kernel is chosen only for 16-byte aligned in0 / out / weight / scale / shift, as in a launch. */
int v2x_conv2d_plan(const v2x_conv_desc *desc, char *buf, size_t cap);
/* second(first(x)) for two consecutive HBM-bound layers with the intermediate map kept on chip (conv_halo_pair.hip):
 * replaces Backbone.py::LidarEncoder's conv_pre_1 + bn + relu + conv_pre_2 + bn + relu.  Both descriptors: 3x3, stride 1,
 * pad 1, w_layout 1, C0 = 32 (13 real + zero-weight padding for the first), C1 = 0, Cout = 32, bf16 epilogue;
 * first->in_format = 1 (bit grid, in_zbits <= 16); H % 8 == 0, W % 32 == 0.  first->out is ignored; the result is
 * bit-identical to v2x_conv2d(first) followed by v2x_conv2d(second).
 * SECOND FORM (ABI 16; selected by second->Cout2 > 0 with first->in_format = 0) -- the detection tail, conv_tail.hip: replaces
 * Backbone.py::LidarDecoder's conv8_2 + bn + relu followed by DetModelBase.py's ClassificationHead and SingleRegressionHead.
 * first = conv8_2 (3x3, stride 1, pad 1, w_layout 1, C0 = 32, C1 = 0, Cout = 32, bf16 epilogue, in0 = conv8_1's output, bf16 NHWC [N][H][W][32]);
 * second = the fused heads exactly as v2x_conv2d takes them (w_layout 1, C0 = 32, Cout = 64 hidden rows in chain order, Cout2 = 48, weight2 / scale2 /
 * shift2, relu2 = 0, epilogue V2X_EPI_F32, split = the classification channels (4, 8 or 12), out / out2 16-byte aligned).  H % 8 == 0, W % 32 == 0, N H W < 2^27.  conv8_2's
 * output is never stored (first->out ignored); the logits are bit-identical to v2x_conv2d(first) followed by v2x_conv2d(second). */
int v2x_conv2d_pair(const v2x_conv_desc *first, const v2x_conv_desc *second, v2x_stream_t stream);

/* ---------------------------------------------------------------- communication codec (compress_level = k; codec.hip)
 * Upstream Backbone.py::LidarEncoder with compress_level = k > 0 wraps the transmitted map x_3 in com_compresser / bn_compress / ReLU and
 * com_decompresser / bn_decompress / ReLU (two 1x1 Conv2d, C -> Cc = C >> k -> C); DESIGN.md section 3 freezes the specification.
 *     msg[p][:] = relu(scale_c * (Wc x[p][:]) + shift_c)  rounded to bf16  -- the MESSAGE an agent sends: [M][Cc] bf16, natural channel order
 *     y[p][:]   = relu(scale_d * (Wd msg[p][:]) + shift_d) rounded to bf16
 * x, y: [M][C] bf16 NHWC pixels, C = 128 or 256, Cc a power of two in [1, C / 2], 0 < M < 2^31 - 64 (any M: no multiple of 16 needed); every pointer
 * 16-byte aligned.  v2x_codec_1x1 does both in one launch, the message stays in registers and goes to `msg` only when msg != NULL;
 * v2x_codec_compress is the sender's half, v2x_codec_decompress the receiver's.  decompress(compress(x)) is BIT-IDENTICAL to the fused launch, and
 * the bits of a pixel depend on that pixel alone (not on M or on its position in the launch).  fp32 accumulation over ascending 32-channel chunks.
 * Weights: one packed buffer of MFMA A fragments, [fragment][lane = 16 q + j][8] bf16, CT1 = max(Cc / 16, 1), KS2 = max(Cc / 32, 1):
 *     stage one, fragments (i, ks), i < CT1, ks < C / 32:   element e = Wc[16 i + j][32 ks + 8 q + e]            (rows >= Cc are zero)
 *     stage two, fragments (i, c),  i < C / 16, c < KS2:    element e = 4 h + r = Wd[16 i + j][32 c + 16 h + 4 q + r]   (columns >= Cc are zero)
 * -- stage two's K slots are in the chain order of stage one's accumulators ("weight layouts" above), so the message feeds it from registers.
 * Then fp32 `ss`: scale_c[16 CT1], shift_c[16 CT1] (padding rows 1 / 0), scale_d[C], shift_d[C].  v2x_pack_codec_size -> bf16 elements of the
 * weight buffer (and the floats of `ss`), or V2X_EINVAL (the same C and Cc as the launches); v2x_pack_codec runs on the HOST: wc [Cc][C], wd [C][Cc] fp32 row-major. */
long long v2x_pack_codec_size(int C, int Cc, long long *ss_floats);
int v2x_pack_codec(int C, int Cc, const float *wc, const float *scale_c, const float *shift_c, const float *wd, const float *scale_d,
                   const float *shift_d, uint16_t *dst_w, float *dst_ss);
int v2x_codec_1x1(const uint16_t *x, long long M, int C, int Cc, const uint16_t *wpack, const float *sspack, uint16_t *y, uint16_t *msg,
                  v2x_stream_t stream);
int v2x_codec_compress(const uint16_t *x, long long M, int C, int Cc, const uint16_t *wpack, const float *sspack, uint16_t *msg,
                       v2x_stream_t stream);
int v2x_codec_decompress(const uint16_t *msg, long long M, int C, int Cc, const uint16_t *wpack, const float *sspack, uint16_t *y,
                         v2x_stream_t stream);

/* ---------------------------------------------------------------- f-3: backward of the 3x3 stride-1 convolutions
 * Upstream trains through torch.autograd (cuDNN / MIOpen kernels behind nn.Conv2d.backward, tools/det/train_codet.py).
 *   data gradient:   dX = conv3x3(dY, W') with W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx] -- a forward convolution: v2x_conv2d
 *                    on the re-packed weights (v2x_sim_amd/train/hip_conv.py);
 *   weight gradient: v2x_conv3x3_wgrad, an MFMA kernel contracting over pixels (conv_wgrad.hip).
 * x bf16 NHWC [N][H][W][Cin], dy bf16 NHWC [N][H][W][Cout]; H % 8 == 0, W % 32 == 0, Cin % 32 == 0, Cout % 32 == 0.
 * workspace fp32 [n_split][Cout][3][3][Cin]: partial sums, every element written; dW = sum over the first axis (the caller
 * adds them in a fixed order: deterministic).  Cout % 64 == 0: n_split in [1, number of 8x32 pixel tiles]; otherwise (the 32-row
 * form, two workspace slots per block) n_split even, in [2, 2 x tiles].  v2x_conv3x3_wgrad_splits gives the library's choice
 * (0 = unsupported shape).  Stride-2 layers: pass dy with zeros inserted between its pixels (dy_z[2y][2x] = dy[y][x]) and the
 * layer's input x -- the same sum (v2x_sim_amd/train/hip_conv.py). */
int v2x_conv3x3_wgrad_splits(int N, int H, int W, int Cin, int Cout);
int v2x_conv3x3_wgrad(const uint16_t *x, const uint16_t *dy, int N, int H, int W, int Cin, int Cout, float *workspace,
                      int n_split, v2x_stream_t stream);
/* The fixed-order sum of the partials, written in the parameter's own layout: dw_oihw fp32 [Cout][cin_out][3][3] =
 * sum_s workspace[s][co][ky][kx][ci] for ci < cin_out <= Cin (cin_out < Cin: the layer's input was stored zero-padded). */
int v2x_conv3x3_wgrad_reduce(const float *workspace, int n_split, int Cout, int Cin, int cin_out, float *dw_oihw, v2x_stream_t stream);

/* ---------------------------------------------------------------- f-3: batch-statistics BatchNorm + ReLU on bf16 NHWC maps
 * Replaces nn.BatchNorm2d / nn.BatchNorm3d in TRAIN mode followed by F.relu as Backbone.py applies them after every convolution
 * (`F.relu(self.bn1_1(self.conv1_1(x)))`), forward and backward (bn_train.hip).  x [M][C] bf16 with M = N*H*W pixels: the
 * convolution's output as v2x_conv2d wrote it.  C / 8 must divide 256 (C = 8, 16, 32, ..., 2048).
 *   forward:  mean / biased variance over the M pixels (fp32 partials, fp64 finish, fixed order), y = relu((x - mean) * invstd *
 *             gamma + beta) -> bf16; save_mean / save_invstd [C] for the backward; running_mean / running_var (both or neither)
 *             updated as nn.BatchNorm does (momentum, unbiased variance).  relu = 0 leaves the ReLU out.
 *   backward: g = dy * [y > 0] (y recomputed from x), dbeta = sum g, dgamma = sum g * xhat,
 *             dx = gamma * invstd * (g - dbeta / M - xhat * dgamma / M) -> bf16.
 * workspace: v2x_bn_train_workspace_size(M, C) bytes of device memory (per-workgroup partial sums; 0 = unsupported shape).
 * No atomics: results are bit-reproducible run to run. */
long long v2x_bn_train_workspace_size(long long M, int C);
int v2x_bn_train_forward(const uint16_t *x, long long M, int C, const float *gamma, const float *beta, float eps, float momentum,
                         float *running_mean, float *running_var, int relu, uint16_t *y, float *save_mean, float *save_invstd,
                         float *workspace, v2x_stream_t stream);
int v2x_bn_train_backward(const uint16_t *x, const uint16_t *dy, long long M, int C, const float *gamma, const float *beta,
                          const float *save_mean, const float *save_invstd, int relu, uint16_t *dx, float *dgamma, float *dbeta,
                          float *workspace, v2x_stream_t stream);
/* The same, and dx_sum[c] = the sum over the M pixels of dx as stored (bf16-rounded), fp32 [C]: the bias gradient of the convolution whose
 * output x is (autograd's reduction in nn.Conv2d.backward), accumulated by the kernel that writes dx instead of a second pass over it.
 * sum_workspace: v2x_bn_dxsum_workspace_size(M, C) bytes.  Fixed summation order. */
long long v2x_bn_dxsum_workspace_size(long long M, int C);
int v2x_bn_train_backward_dxsum(const uint16_t *x, const uint16_t *dy, long long M, int C, const float *gamma, const float *beta,
                                const float *save_mean, const float *save_invstd, int relu, uint16_t *dx, float *dgamma, float *dbeta,
                                float *dx_sum, float *workspace, float *sum_workspace, v2x_stream_t stream);

/* ---------------------------------------------------------------- a3 (+ the sum of a4/a5): warp + fuse
 * Replaces DetModelBase.py::feature_transformation (affine_grid + grid_sample twice,
 * bilinear, zeros, align_corners=False) together with the reduction that consumes
 * it: torch.mean(torch.stack(neighbours)) in V2VNet.py and the attention-weighted
 * sum of MIMOGeneralDotProductAttention in When2com.py.
 *
 * feat:  bf16 NHWC [A*Bt][H][W][C], item index = agent*Bt + frame (agent-major, as the
 *        reference batches agents).
 * trans: fp32 [Bt][A][A][4][4]; trans[f][ego][nb] is the pose used to bring nb into ego.
 * items: int32 [n_out][2] = (ego agent, frame) of every output map (lets a rank fuse only
 *        the items it owns after the all-gather).
 * coef:  fp32 [n_out][A] weight of source agent j for output m (0 = skip). j == ego is
 *        taken unwarped.
 * mode:  V2X_FUSE_WSUM  out = sum_j coef*warp_j ;  V2X_FUSE_MEAN  out = (sum_{coef!=0} warp_j) / count ;
 *        V2X_FUSE_MAX   out = max_{coef!=0} warp_j  (elementwise; the zero padding of a warped map takes part, as in
 *        upstream's torch.max(torch.stack(...)) of MaxFusion)
 * out:   bf16 NHWC [n_out][H][W][C].   C % 8 == 0.   n_out == 0: returns V2X_OK, nothing is launched; items / coef / out may be NULL then. */
enum { V2X_FUSE_WSUM = 0, V2X_FUSE_MEAN = 1, V2X_FUSE_MAX = 2 };
int v2x_warp_fuse(const uint16_t *feat, int A, int Bt, int H, int W, int C, const float *trans,
                  const int32_t *items, int n_out, const float *coef, int mode, uint16_t *out,
                  v2x_stream_t stream);
/* The same launch with its workgroups ordered by FRAME: order int32 [order_len] = the output-map index of (frame slot, ego) in slots of
 * order_stride entries (-1 = none), order_len >= n_out.  The workgroups of XCD x (linear id % 8) compute the slots x, x + 8, ...: the
 * output maps of a frame read the same A source maps, which then cross the fabric once per frame instead of once per ego.  Same arithmetic,
 * identical bits; only the LDS-staged form (H, W multiples of 8, C of 128) uses the table, the direct form ignores it. */
int v2x_warp_fuse_ordered(const uint16_t *feat, int A, int Bt, int H, int W, int C, const float *trans, const int32_t *items, int n_out,
                          const float *coef, int mode, uint16_t *out, const int32_t *order, int order_stride, int order_len,
                          v2x_stream_t stream);

/* Degraded links (row f-4; DESIGN.md section 3.9 is the frozen rule): this step's fusion plan and poses from the static plan and the clean poses, in
 * ONE launch (one workgroup; no allocation, no host synchronisation, capturable).  p_outage: every directed link j -> i (j != i) is down with that
 * probability, independently; pose_sigma: Gaussian noise of that many metres on the translation of every agent-to-agent transform.
 * Generator: Philox4x32-10.  For the directed pair (ego i, source j) of frame f at step s:
 *   w[0..3] = philox(counter = (s & 0xffffffff, s >> 32, f, (domain << 16) | (i << 8) | j), key = (seed & 0xffffffff, seed >> 32)), A <= 32.
 *   Outage (domain 0): u = float(w[0] >> 8) * 2^-24; the link is down iff u < p_outage.  coef[m][j] = coef0[m][j] for j == ego(m) and for a link
 *     that is not down, 0 otherwise.  p_outage == 0: nothing is drawn, coef = coef0.
 *   Pose (domain 1): u_k = (float(w[k] >> 9) + 0.5) * 2^-23; nx = sqrt(-2 ln u_0) cos(2 pi u_1), ny = sqrt(-2 ln u_0) sin(2 pi u_1),
 *     nz = sqrt(-2 ln u_2) cos(2 pi u_3) in fp32 (libm forms); entries [0][3], [1][3], [2][3] of trans[f][i][j], j != i, become t + pose_sigma * n,
 *     every other entry and the diagonal pairs are copied.  (v2x_warp_fuse reads [0][3] and [1][3].)
 * items int32 [n_out][2] = (ego, frame) as for v2x_warp_fuse; an item outside [0, A) x [0, Bt) keeps its static row and draws nothing.
 * coef0 fp32 [n_out][A]: the static plan's rows, only read.  coef fp32 [n_out][A]: this step's rows.  Both NULL: pose noise alone (p_outage == 0).
 * coef2 fp32 [n_out * A][A] or NULL: DiscoNet's one-hot rows, coef2[m * A + k][j] = (j == k) ? coef[m][k] : 0.
 * link uint8 [Bt][A][A] or NULL: link[f][i][j] = 1 iff j != i and coef[m(i, f)][j] != 0; absent egos and the diagonal are 0.
 * trans fp32 [Bt][A][A][4][4], only read; trans_out the same shape, NULL if and only if pose_sigma == 0 (then trans is not read and may be NULL).
 * step_dev: DEVICE uint64, 8-byte aligned: read as s by every thread, left as s + 1 by the launch's last statement behind a workgroup barrier.
 * Every output element is written.  n_out == 0: nothing to do (V2X_OK), whatever the other arguments are.  p_outage outside [0, 1], pose_sigma
 * negative or not finite, A > 32: V2X_EINVAL. */
int v2x_channel_degrade(const int32_t *items, int n_out, int A, int Bt, const float *coef0, float *coef, float *coef2, uint8_t *link,
                        const float *trans, float *trans_out, float p_outage, float pose_sigma, uint64_t seed, uint64_t *step_dev,
                        v2x_stream_t stream);

/* ---------------------------------------------------------------- a5: attention handshake
 * Replaces When2com.py::MIMOGeneralDotProductAttention (query projection, key.query
 * scores, softmax over the keys) and the inference-time selection
 * (activated_select: threshold 0.2 / argmax_select: top-1).
 *
 * keys:  fp32 [A*Bt][key_size], querys: fp32 [A*Bt][query_size] (agent-major items)
 * w_lin: fp32 [key_size][query_size], b_lin: fp32 [key_size]   (attention_net.linear)
 * prob:  fp32 [Bt][A(k)][A(q)] softmax scores;  coef: same shape after selection
 * mode:  0 softmax (training / 'softmax'), 1 'activated' (coef = p * (p > thres)), 2 'argmax_test' */
int v2x_attn_handshake(const float *keys, const float *querys, const float *w_lin, const float *b_lin, int A,
                       int Bt, int key_size, int query_size, int mode, float thres, float *prob, float *coef,
                       v2x_stream_t stream);

/* The same launch with the normalisation over the keys chosen by `norm`: 0 = softmax (v2x_attn_handshake's bits), 1 = sparsemax
 * (When2com(sparse=True)): per query, with the scores z sorted descending, k* = max{ j : 1 + j z_(j) > sum_{i<=j} z_(i) },
 * tau = (sum_{i<=k*} z_(i) - 1) / k*, prob_k = max(z_k - tau, 0) -- the projection of the score column onto the simplex, exact zeros
 * outside its support.  The selections act on prob as above (the first maximum wins 'argmax_test').  Any other norm: V2X_EINVAL. */
int v2x_attn_handshake_norm(const float *keys, const float *querys, const float *w_lin, const float *b_lin, int A,
                            int Bt, int key_size, int query_size, int mode, int norm, float thres, float *prob,
                            float *coef, v2x_stream_t stream);

/* ---------------------------------------------------------------- a8: seg argmax + confusion matrix
 * logits fp32 NHWC [n][H][W][n_cls]; label uint8 [n][H][W]; pred uint8 [n][H][W] (may be NULL);
 * conf int64 [n_cls][n_cls] (rows = label, cols = prediction), accumulated (caller zeroes). */
int v2x_seg_argmax_confusion(const float *logits, const uint8_t *label, int n, int H, int W, int n_cls,
                             uint8_t *pred, long long *conf, v2x_stream_t stream);

/* ---------------------------------------------------------------- f-4 (DiscoNet): per-pixel softmax-weighted fusion
 * Replaces the tail of coperception/models/det/DiscoNet.py::fusion.  scores fp32 [n_items][A][H][W][score_stride] (channel 0
 * = the ReLU'd 1-channel output of PixelWeightedFusionSoftmax for source k), valid fp32 [n_items][A] (0 = source absent),
 * maps bf16 [n_items][A][H][W][C] (source k warped into the ego frame) -> out bf16 [n_items][H][W][C]:
 * w_k = exp(s_k) / sum_j exp(s_j) per pixel, out = sum_k w_k * map_k. */
int v2x_pixel_weighted_fuse(const float *scores, int score_stride, const float *valid, const uint16_t *maps, int n_items,
                            int A, int H, int W, int C, uint16_t *out, v2x_stream_t stream);

/* Per-channel sum of a bf16 [M][C] map -> fp32 [C]: the bias gradient of a convolution (db = dy summed over batch and pixels;
 * upstream: autograd's sum inside nn.Conv2d.backward).  Fixed summation order (bit-reproducible).  C as for the BN entries;
 * workspace: v2x_channel_sum_workspace_size(M, C) bytes (0 = unsupported shape). */
long long v2x_channel_sum_workspace_size(long long M, int C);
int v2x_channel_sum_bf16(const uint16_t *x, long long M, int C, float *out, float *workspace, v2x_stream_t stream);

/* Row f-3 (ABI 17): the gradient of a 1x1 head arriving from the loss -- fp32 [M][C] (C % 4 == 0: 12 class logits, 36 box codes per pixel) -- made ready
 * for the data- and weight-gradient kernels in ONE pass: out = the same values as bf16 [M][Cp], channels C..Cp-1 zero (Cp % 8 == 0, Cp >= C, Cp / 8 divides
 * 256), and sums[c] = the per-channel sum over the M pixels of the fp32 values (the layer's bias gradient; fixed summation order, bit-reproducible).
 * Replaces, in upstream's terms, autograd's pad / cast / sum around nn.Conv2d.backward of ClassificationHead.conv2 and the regression head's last conv
 * (coperception/models/det/base/DetModelBase.py, not in /root/reference): six PyTorch-op launches and four passes over the logit gradients per head.
 * workspace: v2x_cast_pad_chsum_workspace_size(M, Cp) bytes (0 = unsupported shape). */
long long v2x_cast_pad_chsum_workspace_size(long long M, int Cp);
int v2x_cast_pad_chsum_f32(const float *x, long long M, int C, int Cp, uint16_t *out, float *sums, float *workspace, v2x_stream_t stream);

/* Row f-3, the detection loss of a training step, forward and backward (replaces coperception/utils/loss.py's SoftmaxFocalClassificationLoss +
 * WeightedSmoothL1LocalizationLoss as combined by coperception/utils/CoDetModule.py::FaFModule.loss_calculator -- not in /root/reference,
 * README.md:101 names the scripts that call them; restated in v2x_sim_amd/train/loss.py): DEVICE fp32 cls [n][2] logits, labels [n][2] one-hot,
 * loc / targets [n][6] box codes, mask [n] bytes (bool).  cls = sum -alpha_t (1 - p_t)^2 sum_k l_k log softmax(cls)_k with alpha_t = alpha l_1 +
 * (1 - alpha) l_0; loc = sum over masked anchors of smooth-L1 (beta); out4 = {cls / n + loc / n, cls / n, loc / n, n = max(sum l_1, 1)}.
 * Forward = two launches (per-workgroup partials in workspace -- v2x_det_loss_workspace_size(n) bytes -- added in a fixed order: bit-reproducible);
 * backward = one launch writing dcls [n][2] and dloc [n][6] for the incoming gradients of the three outputs (DEVICE scalars, NULL = 0). */
/* Row f-3, the ConvGRU's gate arithmetic in the training graph (convolutional_rnn.Conv2dGRU with hidden = None as V2VNet.py calls it; restated in
 * v2x_sim_amd/train/graph.py::_gru_step): gi fp32 [P][3C][HW] = the input convolution's output (bias_ih included), bias_hh fp32 [3C] ->
 * h fp32 [P][C][HW] = n - z n with r = sigmoid(gi_r + bh_r), z = sigmoid(gi_z + bh_z), n = tanh(gi_n + r bh_n).  Backward: dh -> dgi [P][3C][HW]
 * and dn_r [P][C][HW] = d(pre-activation of n) * r; d bias_hh = (channel sums of dgi's r and z planes, channel sums of dn_r).  HW % 4 == 0. */
int v2x_gru_gates_f32(const float *gi, const float *bias_hh, long long P, int C, int HW, float *h, v2x_stream_t stream);
int v2x_gru_gates_bwd_f32(const float *gi, const float *bias_hh, const float *dh, long long P, int C, int HW, float *dgi, float *dn_r,
                          v2x_stream_t stream);
long long v2x_det_loss_workspace_size(long long n_anchors);
int v2x_det_loss_forward(const float *cls, const float *labels, const float *loc, const float *targets, const uint8_t *mask, long long n_anchors,
                         float alpha, float beta, float *out4, float *workspace, v2x_stream_t stream);
int v2x_det_loss_backward(const float *cls, const float *labels, const float *loc, const float *targets, const uint8_t *mask, long long n_anchors,
                          float alpha, float beta, const float *out4, const float *g_loss, const float *g_cls, const float *g_loc, float *dcls,
                          float *dloc, v2x_stream_t stream);
/* Row f-3, the same loss with the CORNER form of the localisation term (coperception/utils/CoDetModule.py::FaFModule.loss_calculator under
 * config.loss_type = "corner_loss" -- not in /root/reference; DESIGN.md section 3.10 is the build-owned specification, restated in
 * v2x_sim_amd/train/loss.py::detection_loss and at the head of csrc/det_corner_loss.hip).  Operands as v2x_det_loss_forward, plus anchors: DEVICE fp32
 * [anchors_per_map][6] (x, y, w, h, sin, cos), 8-byte aligned; anchor i decodes through row i mod anchors_per_map, and n_anchors must be a multiple of
 * anchors_per_map (V2X_EINVAL + v2x_last_error otherwise).  loc = sum over masked anchors of sum_k |corner_k(decode(loc_i)) - corner_k(decode(targets_i))|_2
 * with the 'faf' decode (w = wa exp(clip(dw, -4, 4)), yaw = atan2(sa, ca) + atan2(ds, dc), 0 at ds = dc = 0) and box_corners' corner order; wh_swap != 0:
 * h runs along the heading (Config.box_wh_axis = "h_along_heading").  The codes of an unmasked anchor are not read (inf / NaN there change nothing; its
 * dloc row is 0); |D| = 0, ds = dc = 0 and a clipped dw / dh give gradient 0.  cls, out4 = {cls / n + loc / n, cls / n, loc / n, n = max(sum l_1, 1)},
 * the workspace (v2x_det_loss_workspace_size(n_anchors) bytes), the launches (two forward, one backward; fixed order, bit-reproducible, capturable) and the
 * incoming gradients (DEVICE scalars, NULL = 0) are v2x_det_loss_forward / _backward's. */
int v2x_det_corner_loss_forward(const float *cls, const float *labels, const float *loc, const float *targets, const uint8_t *mask, const float *anchors,
                                long long n_anchors, long long anchors_per_map, int wh_swap, float alpha, float *out4, float *workspace,
                                v2x_stream_t stream);
int v2x_det_corner_loss_backward(const float *cls, const float *labels, const float *loc, const float *targets, const uint8_t *mask, const float *anchors,
                                 long long n_anchors, long long anchors_per_map, int wh_swap, float alpha, const float *out4, const float *g_loss,
                                 const float *g_cls, const float *g_loc, float *dcls, float *dloc, v2x_stream_t stream);

/* Rows a8 / f-3, the segmentation loss of a training step, forward and backward (replaces the nn.CrossEntropyLoss of
 * coperception/utils/SegModule.py::SegModule.step and its autograd backward -- not in /root/reference, README.md:101 names the scripts that call it;
 * restated in v2x_sim_amd/train/loss.py::segmentation_loss): DEVICE fp32 logits [M][C] (NHWC, C % 4 == 0, 4 <= C <= 32, 16-byte aligned), labels
 * [M] bytes, weight fp32 [C] or NULL (= 1).  A label >= C is ignored (255 by convention): w_i = label_i < C ? weight[label_i] : 0;
 * num = sum w_i (logsumexp(logits_i) - logits_i[label_i]), den = sum w_i, out3 = {num / (den > 0 ? den : 1), num, den} -- F.cross_entropy(weight=,
 * ignore_index=, reduction="mean") wherever den > 0, and 0 with zero gradients (not NaN) when every pixel is ignored.
 * Forward = two launches (per-workgroup partials in workspace, added in workgroup order in fp64: bit-reproducible).
 * Backward = d loss / d logit_ij = g w_i (softmax_ij - [j == label_i]) / den with g (g_loss: a DEVICE scalar, NULL = 1) and den (out3) read on the
 * device, in two output forms over one per-pixel function -- the same values before rounding:
 *   v2x_seg_loss_backward         one launch: dlogits fp32 [M][C];
 *   v2x_seg_loss_backward_packed  two launches: what v2x_cast_pad_chsum_f32 would make of dlogits -- dy bf16 [M][Cp] (Cp by that entry's rules: Cp >= C,
 *                                 Cp % 8 == 0, Cp / 8 divides 256; channels C..Cp-1 zero; bit-equal to the cast of the first form) and sums fp32 [C],
 *                                 the per-channel sums of the fp32 gradients (the class head's bias gradient; fixed order: bit-reproducible).  The fp32
 *                                 gradient is never stored.
 * No atomics; every output is bit-reproducible.  workspace: v2x_seg_loss_workspace_size(M, C, Cp) bytes covers the forward and the packed backward
 * (Cp = 0: the forward alone); 0 = unsupported shape. */
long long v2x_seg_loss_workspace_size(long long M, int C, int Cp);
int v2x_seg_loss_forward(const float *logits, const uint8_t *labels, const float *weight, long long M, int C, float *out3, float *workspace,
                         v2x_stream_t stream);
int v2x_seg_loss_backward(const float *logits, const uint8_t *labels, const float *weight, long long M, int C, const float *out3, const float *g_loss,
                          float *dlogits, v2x_stream_t stream);
int v2x_seg_loss_backward_packed(const float *logits, const uint8_t *labels, const float *weight, long long M, int C, const float *out3,
                                 const float *g_loss, int Cp, uint16_t *dy, float *sums, float *workspace, v2x_stream_t stream);

/* ---------------------------------------------------------------- f-3: the cross-agent warp of the TRAINING graph, forward and data gradient
 * Replaces F.affine_grid + F.grid_sample(mode="bilinear", padding_mode="zeros", align_corners=False) of
 * coperception/models/det/base/IntermediateModelBase.py::feature_transformation (applied twice there: rotation, then translation) and its
 * autograd backward.  in / out fp32 [P][C][H][W] (the fusion stage of the training graph is fp32 NCHW), theta fp32 [P][2][3] (the matrices
 * F.affine_grid takes).  v2x_warp_affine_bwd_f32 is the exact transpose of v2x_warp_affine_f32 with respect to `in` (theta carries no
 * gradient: poses are data), computed as a gather in a fixed order -- bit-reproducible, unlike the atomic scatter of
 * grid_sampler_2d_backward.  Agreement with torch: fp32 rounding of the coordinate arithmetic (tests/test_gpu_train_kernels.py). */
int v2x_warp_affine_f32(const float *in, const float *theta, int P, int C, int H, int W, float *out, v2x_stream_t stream);
int v2x_warp_affine_bwd_f32(const float *dout, const float *theta, int P, int C, int H, int W, float *din, v2x_stream_t stream);

/* f-3 (round 6): V2VNet's message-passing round of the TRAINING graph on bf16 NHWC maps -- no layout or precision change around the fusion stage.
 * Replaces, of coperception/models/det/V2VNet.py::forward (not in /root/reference; README.md:101 names the model; restated in
 * v2x_sim_amd/train/graph.py::v2v_fuse): the per-pair index_select, the two feature_transformation passes (F.affine_grid + F.grid_sample: rotation
 * about the map centre, then translation by (4 T03 / 128, -4 T13 / 128)), the mean over an ego's K neighbours and torch.cat([ego, mean], 1) -- and
 * their autograd backward.  Every item m = 0 .. M-1 has exactly K pairs, consecutive (pair = m K + k).
 *   v2x_v2v_message_bf16: cur, base bf16 [N][H][W][C] (the ego maps; the maps the neighbours send -- the same pointer unless a later round sends the
 *     un-updated maps), trans fp32 [*][4][4], src / tsel int32 [M K] (a pair's row of base / matrix of trans), rows int32 [M] (item m's row of cur)
 *     -> conv_in bf16 [M][H][W][2C] = [cur[rows[m]] | mean_k warp2(base[src[m K + k]])].  The two resampling passes are evaluated without the
 *     intermediate map, with the arithmetic and the order of additions of v2x_warp_affine_f32 applied twice (fp32; one bf16 rounding at the store).
 *   v2x_v2v_message_bwd_bf16: dconv_in bf16 [M][H][W][2C], inv int32 [N][K] (the pairs that read row r of base, in pair order), item_of_row int32 [N]
 *     (the item whose ego map row r is, or -1) -> dbase bf16 [N][H][W][C], the exact transpose (a gather over both passes' candidate pixels in a
 *     fixed order: bit-reproducible); dcur = NULL: the ego half is added into dbase (base == cur), else it is written to dcur [N][H][W][C].
 * The ConvGRU's gates on bf16 NHWC (the arithmetic of v2x_gru_gates_f32): gi bf16 [P][3C] (P = maps x pixels), bias_hh fp32 [3C] -> h bf16 [P][C];
 * backward: dh bf16 [P][C] -> dgi bf16 [P][3C] and sums6c fp32 [6C] = (channel sums of dgi AS STORED: r, z, n = d bias_ih of the input convolution |
 * the r and z sums again, the sums of d(pre-activation of n) * r = d bias_hh), per-workgroup partials in workspace
 * (v2x_gru_gates_nhwc_workspace_size bytes; 0 = unsupported shape) added in a fixed order.  C / 8 must divide 256. */
int v2x_v2v_message_bf16(const uint16_t *cur, const uint16_t *base, const float *trans, const int *src, const int *tsel, const int *rows, int M, int K, int N,
                         int C, int H, int W, uint16_t *conv_in, v2x_stream_t stream);
int v2x_v2v_message_bwd_bf16(const uint16_t *dconv_in, const float *trans, const int *inv, const int *tsel, const int *item_of_row, int M, int K, int N, int C,
                             int H, int W, uint16_t *dbase, uint16_t *dcur, v2x_stream_t stream);
int v2x_gru_gates_nhwc_bf16(const uint16_t *gi, const float *bias_hh, long long P, int C, uint16_t *h, v2x_stream_t stream);
long long v2x_gru_gates_nhwc_workspace_size(long long P, int C);
int v2x_gru_gates_nhwc_bwd_bf16(const uint16_t *gi, const float *bias_hh, const uint16_t *dh, long long P, int C, uint16_t *dgi, float *sums6c,
                                float *workspace, v2x_stream_t stream);

/* f-3 (round 6): the optimizer step.  Adam with torch.optim.Adam's arithmetic (the optimizer upstream's train scripts build, README.md:101:
 *     g = grad (+ weight_decay p);  m += (1 - beta1)(g - m);  v = beta2 v + (1 - beta2) g g;  p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps))
 * over up to V2X_ADAM_MAX_TENSORS parameter tensors in ONE launch.  `tensors` is a HOST table of DEVICE fp32 pointers (it travels in the kernel
 * arguments: nothing is uploaded, the launch is capturable); step[i] = the tensor's DEVICE step counter t, already incremented (capturable optimizers),
 * or NULL: t = step_host.  lr_dev = a DEVICE learning rate or NULL: lr.  The hyper-parameters are doubles, as Python holds them: 1 - beta and 1 - beta^t
 * are formed in fp64 ((float)0.999 is 1.3e-5 away from 0.999 in 1 - beta2^t), the per-element arithmetic is fp32.  Tensors with numel 0 are skipped. */
#define V2X_ADAM_MAX_TENSORS 72
typedef struct v2x_adam_tensors {
    float *param[V2X_ADAM_MAX_TENSORS];
    const float *grad[V2X_ADAM_MAX_TENSORS];
    float *exp_avg[V2X_ADAM_MAX_TENSORS];
    float *exp_avg_sq[V2X_ADAM_MAX_TENSORS];
    const float *step[V2X_ADAM_MAX_TENSORS];
    long long numel[V2X_ADAM_MAX_TENSORS];
} v2x_adam_tensors;
int v2x_adam_step_f32(const v2x_adam_tensors *tensors, int n_tensors, const float *lr_dev, double lr, double beta1, double beta2, double eps, double weight_decay,
                      double step_host, v2x_stream_t stream);

/* f-3: the decoder's up + concat of the TRAINING graph and its backward (the inference kernels fold it into their loaders: v2x_conv_desc.up0).
 * Replaces torch.cat((F.interpolate(x, scale_factor=(2, 2)), skip), dim=1) of Backbone.py::LidarDecoder and its autograd backward.
 * lo bf16 [N][H][W][C0] (H, W = the LOW-resolution extent), skip bf16 [N][2H][2W][C1] -> out bf16 [N][2H][2W][C0 + C1] (lo's channels first).
 * Backward: dcat bf16 [N][2H][2W][C0 + C1] -> d_lo [N][H][W][C0] = the 2x2 sums (fp32, row-major order, rounded once), d_skip [N][2H][2W][C1].
 * C0, C1 multiples of 8. */
int v2x_upcat_bf16(const uint16_t *lo, const uint16_t *skip, int N, int H, int W, int C0, int C1, uint16_t *out, v2x_stream_t stream);
int v2x_upcat_bwd_bf16(const uint16_t *dcat, int N, int H, int W, int C0, int C1, uint16_t *d_lo, uint16_t *d_skip, v2x_stream_t stream);
/* f-3: dy bf16 [N][Ho][Wo][C] of a stride-2 layer -> out bf16 [N][2Ho][2Wo][C] with dy at the even positions and zeros elsewhere (the operand of
 * the layer's data and weight gradients as stride-1 computations; replaces torch.zeros + a strided copy).  C % 8 == 0. */
int v2x_zero_insert_bf16(const uint16_t *dy, int N, int Ho, int Wo, int C, uint16_t *out, v2x_stream_t stream);

/* ---------------------------------------------------------------- f-1: detection post-processing
 * Replaces coperception/utils/postprocess.py::apply_nms_det per (agent, frame) map: foreground softmax score, score
 * threshold, 'faf' anchor decode (x, y, w, h, yaw) and greedy NMS on the axis-aligned stand-up boxes, in
 * (score descending, anchor index ascending) order.
 *
 * cls: fp32 [n][M][2] logits;  loc: fp32 [n][M][6] box codes;  anchors: fp32 [M][6] (x, y, w, h, sin, cos), M = X*Y*A.
 * cap: candidate capacity per map, a power of two in [64, 4096].
 * out_boxes fp32 [n][cap][5], out_scores fp32 [n][cap], out_index int32 [n][cap] (anchor index of each detection),
 * out_count int32 [n]: number of detections of map i, or -(number of candidates) when more than `cap` anchors passed the
 * threshold (nothing else is written for that map: the caller retries with a higher threshold or post-processes on the host).
 * Entries >= out_count of out_scores and out_index are not written; rows >= out_count of out_boxes are the call's staging area (the decoded
 * candidates, kept ones compacted to the front afterwards): their contents are unspecified.  The caller clears nothing.
 * key_scratch: uint64 [n][cap], count_scratch: int32 [n] (caller-owned workspace; cleared and written by the call). */
int v2x_det_postprocess(const float *cls, const float *loc, const float *anchors, int n, int M, float score_thr,
                        float nms_thr, int cap, float *out_boxes, float *out_scores, int32_t *out_index,
                        int32_t *out_count, unsigned long long *key_scratch, int32_t *count_scratch,
                        v2x_stream_t stream);

/* Same, but the greedy suppression compares the ROTATED boxes (convex-polygon IoU in fp64; the stand-up overlap is only the
 * cheap reject).  Upstream's apply_nms_det suppresses on stand-up boxes (v2x_det_postprocess); this is the variant SURVEY.md
 * row f-1 lists ("rotated-box NMS"). */
int v2x_det_postprocess_rotated(const float *cls, const float *loc, const float *anchors, int n, int M, float score_thr,
                                float nms_thr, int cap, float *out_boxes, float *out_scores, int32_t *out_index,
                                int32_t *out_count, unsigned long long *key_scratch, int32_t *count_scratch,
                                v2x_stream_t stream);

/* The second half of the two above for candidates that a V2X_EPI_DET launch of v2x_conv2d already selected (the logits never
 * reach memory: apply_nms_det's softmax + threshold run in the heads' epilogue).  keys uint64 [n][cap], codes fp32 [n][cap][6],
 * counts int32 [n] exactly as that launch wrote them; everything else as v2x_det_postprocess (rotated != 0: the rotated-box
 * variant).  Same detections, bit for bit, as v2x_det_postprocess on the logits the heads would have written. */
int v2x_det_nms_candidates(const unsigned long long *keys, const float *codes, const int32_t *counts, const float *anchors, int n,
                           int M, int cap, float nms_thr, int rotated, float *out_boxes, float *out_scores, int32_t *out_index,
                           int32_t *out_count, v2x_stream_t stream);

/* Late fusion (upstream test_codet.py --com late, the paper's "Co-lower-bound"): the agents exchange their DETECTIONS; every ego moves its
 * neighbours' boxes into its own frame and suppresses the union.  One workgroup per ego, all A*B egos of the call, at most two launches
 * (as the NMS above: the second takes the egos with more than 512 merged candidates); no allocation, no host synchronisation.
 * boxes fp32 [A*B][cap_in][5], scores fp32 [A*B][cap_in], counts int32 [A*B]: what v2x_det_postprocess / v2x_det_nms_candidates wrote, rows
 *   agent-major (row of agent j in frame b = j*B + b).  A count above cap_in reads as cap_in.
 * rigid fp32 [B][A][A][8]: entry (b, i, j) = (r00, r01, tx, r10, r11, ty, dyaw, 0) moves a box of agent j into ego i's frame:
 *   x' = (r00*x + r01*y) + tx, y' = (r10*x + r11*y) + ty, yaw' = yaw + dyaw in fp32, every product and sum rounded on its own; w, h stay.
 *   (From the dataset's trans_matrices: r = T[0:2, 0:2], tx = T13, ty = -T03, dyaw = atan2(T10, T00): utils/postprocess.late_rigid_from_trans.)
 * link uint8 [B][A][A]: ego i of frame b receives from j; the diagonal says whether i itself is present (0: out_count 0).
 * The ego's own detections enter bit for bit and uncropped; a neighbour's enter iff x_lo <= x' < x_hi and y_lo <= y' < y_hi.  A candidate with a
 * non-finite field (score included) or a score that is not >= 0 is dropped.  Order: score descending; ties: the ego's own boxes, then neighbours by
 * ascending agent index, then by ascending rank in the source list.  Suppression: exactly v2x_det_postprocess's (rotated != 0: _rotated's).
 * out_boxes fp32 [A*B][cap_out][5], out_scores fp32 [A*B][cap_out] (the source's bits), out_src int32 [A*B][cap_out] = j*cap_in + rank of the
 * source, out_count int32 [A*B]; negative = not computed: -(merged candidates) when they exceed cap_out, -(cap_out + 1) when the ego or a
 * linked source carried a negative count itself.  cap_in, cap_out: powers of two in [64, 4096].  A*B == 0: nothing to do (V2X_OK).
 * Entries >= out_count of out_scores and out_src are not written; rows >= out_count of out_boxes are staging area, contents unspecified. */
int v2x_det_late_fuse(const float *boxes, const float *scores, const int32_t *counts, int A, int B, int cap_in,
                      const float *rigid, const uint8_t *link, float x_lo, float x_hi, float y_lo, float y_hi,
                      float nms_thr, int rotated, int cap_out, float *out_boxes, float *out_scores,
                      int32_t *out_src, int32_t *out_count, v2x_stream_t stream);

/* f-3: detection training targets -- anchors assigned to ground-truth boxes by rotated IoU with thresholds (upstream assigns when the data is created
 * and stores gt_max_iou; DESIGN.md section 3.7 "IoU assignment" is the frozen rule).  All n_items items of the call in two launches (a workgroup per
 * 16 x 16 tile of cells and item, then a workgroup per item); no atomics, no allocation, no host synchronisation, capturable; EVERY output element is
 * written, the caller clears nothing.
 * gt_boxes fp32 [n_items][gt_cap][5] (x, y, w, h, yaw), gt_count int32 [n_items] (clamped to [0, gt_cap]), gt_cap in [1, 256].  A box with a non-finite
 *   field or a negative extent is dropped; a zero extent is valid and has IoU 0 with everything (v2x_rotated_iou's rule).
 * anchors fp32 [X][Y][A][6] (x, y, w, h, sin, cos): the anchor's box is (x, y, w, h, yaw_a), yaw_a = the fp32 rounding of atan2(sin, cos) in fp64.
 * 0 < neg_thr <= pos_thr <= 1, compared as their fp32 values with the fp64 IoU.  Per anchor q: g* = the valid box of largest IoU (lowest index on ties),
 *   miou that IoU; no box with IoU > 0: g* = -1, miou = 0.  miou >= pos_thr: label (0, 1), mask 1, assoc g*, the code of (q, g*); miou < neg_thr: label
 *   (1, 0), mask 0, assoc -1, code 0; otherwise IGNORED: label (0, 0), mask 0, assoc -1, code 0 (contributes to neither term of v2x_det_loss_forward).
 * Per valid box g with gmax(g) = max over q of IoU(q, g) > 0: gt_max_iou = gmax, gt_best = the lowest flat index (ix*Y + iy)*A + a attaining it; every
 *   other entry of the two (dropped boxes, gmax = 0, at or beyond the count) = 0 and -1.  force_match != 0: anchor gt_best[g] becomes positive for g
 *   whatever the threshold step gave it; several boxes claiming one anchor: the largest IoU wins, the lowest g on ties (anchor_iou stays miou).
 * Code = the inverse of the 'faf' decode: (gx - ax, gy - ay, log(gw/aw), log(gh/ah), sin d, cos d), d = gyaw - yaw_a folded to [-pi/2, pi/2), in fp64
 *   from the fp32 inputs, rounded once.
 * labels fp32 [n][X][Y][A][2], reg_targets fp32 [n][X][Y][A][1][6], reg_loss_mask uint8 [n][X][Y][A][1] (what v2x_det_loss_forward reads); assoc int32
 * [n][X][Y][A] or NULL, anchor_iou fp32 [n][X][Y][A] or NULL; gt_max_iou fp32 [n][gt_cap], gt_best int32 [n][gt_cap].  labels and workspace 8-byte
 * aligned; workspace_bytes >= v2x_det_assign_workspace_size (-1 for sizes out of range: X*Y*A and n_items*tiles must stay below 2^31).
 * n_items == 0: nothing to do (V2X_OK). */
long long v2x_det_assign_workspace_size(long long n_items, int X, int Y, int A, int gt_cap);
int v2x_det_assign_targets(const float *gt_boxes, const int32_t *gt_count, long long n_items, int gt_cap, const float *anchors, int X, int Y, int A,
                           float pos_thr, float neg_thr, int force_match, float *labels, float *reg_targets, uint8_t *reg_loss_mask, int32_t *assoc,
                           float *anchor_iou, float *gt_max_iou, int32_t *gt_best, void *workspace, long long workspace_bytes, v2x_stream_t stream);

/* a8 / f-3: segmentation training targets -- the annotated boxes of every item painted into the per-cell class map bev_seg (upstream's
 * create_data_seg.py does it when the data is created; DESIGN.md section 3.8 "Box rasterization" is the frozen rule).  All n items of the call in at
 * most two launches (a workgroup per 16 x 16 tile of cells and item; with hist, a workgroup per item); no global atomics, no allocation, no host
 * synchronisation, capturable; EVERY output element is written, the caller clears nothing.
 * boxes fp32 [n][cap][5] (x, y, w, h, yaw), cls uint8 [n][cap], count int32 [n] (clamped to [0, cap]), cap in [1, 256].
 * Grid: X x Y cells of vx x vy > 0 from the corner (x0, y0); the centre of cell (i, j) is px = x0 + (i + 0.5) * vx, py = y0 + (j + 0.5) * vy.
 * Coverage: box g covers cell (i, j) iff |lx| <= w/2 and |ly| <= h/2, lx = (px-x)*c + (py-y)*s, ly = -(px-x)*s + (py-y)*c, c = cos(yaw), s = sin(yaw) --
 *   fp64 from the fp32 inputs in exactly that order, every product and sum rounded on its own; borders are closed.  A box with a non-finite field or a
 *   negative extent is dropped; a zero extent is valid (such a box covers a centre only if it lies exactly on it).
 * Winner: among the boxes that cover the cell the greatest rank, the lowest box index on ties.  Class 0 is background and never paints (its boxes are
 *   no-ops); a class c in [1, n_cls) paints c with rank rank[c], or c itself when rank is NULL (a higher id paints over a lower one); a class >= n_cls
 *   paints the ignore label 255 and outranks every class.  An uncovered cell is 0.  n_cls in [2, 32]; rank uint8 [n_cls] or NULL.
 * labels uint8 [n][X][Y] (what v2x_seg_loss_* and v2x_seg_argmax_confusion read); owner int32 [n][X][Y] or NULL: the winning box's index in its item's
 *   list (dropped boxes keep their places), -1 where none; hist int64 [n][n_cls + 1] or NULL: cells per label, the last column counts 255.
 * workspace: needed with hist only; DEVICE, 4-byte aligned, workspace_bytes >= v2x_seg_rasterize_workspace_size (-1 for sizes out of range); it needs no
 *   initialisation.  n * tiles must stay below 2^31.  n == 0: nothing to do (V2X_OK), whatever the other arguments are. */
long long v2x_seg_rasterize_workspace_size(long long n, int X, int Y, int n_cls);
int v2x_seg_rasterize(const float *boxes, const uint8_t *cls, const int32_t *count, long long n, int cap, float x0, float y0, float vx, float vy, int X,
                      int Y, int n_cls, const uint8_t *rank, uint8_t *labels, int32_t *owner, long long *hist, void *workspace,
                      long long workspace_bytes, v2x_stream_t stream);

/* f-2 / f-3: synthetic scenes with occlusion -- the sweeps of all agents of all frames of a step ray-cast against a scene of boxes, compacted into the
 * (points, n_pts) form v2x_voxelize_bits reads, with per-box return counts; v2x_lidar_visible_boxes turns the counts into each sweep's ground truth (the
 * num_lidar_pts rule of the real data preparation).  DESIGN.md section 3.12 "LiDAR ray cast" is the frozen rule.  Two launches (one for the ground truth),
 * no allocation, no host synchronisation, capturable; EVERY output element is written, the caller clears nothing; two calls give identical bytes.
 * sensors fp32 [n_sweeps][6] (x, y, z, yaw, cos yaw, sin yaw); frame_of int32 [n_sweeps]: the sweep's frame (outside [0, n_frames): an empty scene).
 * boxes fp32 [n_frames][box_cap][9] (cx, cy, w, h, yaw, cos yaw, sin yaw, z0, z1), w along the box's local x, h along its local y; box_count int32
 *   [n_frames] (clamped to [0, box_cap]), box_cap in [1, 256].  A box with a non-finite field, a negative extent or z1 < z0 is dropped, keeping its index.
 * beam fp32 [n_beams][2] (cos, sin of the elevation), az fp32 [n_az][2] (cos, sin of the azimuth): ray r = b * n_az + a; n_beams * n_az <= 2^24.  The
 *   host passes every angle as its cos / sin pair: no trigonometric function is called for the geometry.
 * Geometry in fp64 from the fp32 inputs, every product and sum rounded on its own: d = (ce*ca, ce*sa, se), world direction w = (c*dx - s*dy, s*dx + c*dy,
 *   dz), origin o = (x, y, z).  Box g by slabs: px = ox - cx, py = oy - cy, lx = px*cg + py*sg, ly = -px*sg + py*cg, ux = wx*cg + wy*sg, uy = -wx*sg +
 *   wy*cg; x in [-w/2, w/2], y in [-h/2, h/2], z in [z0, z1] with lz = oz, uz = dz; from t_near = -inf, t_far = +inf, per axis: u == 0: a miss when l
 *   lies outside the closed slab, otherwise no constraint; u != 0: ta = (lo - l)/u, tb = (hi - l)/u, t_near = max(t_near, min(ta, tb)), t_far =
 *   min(t_far, max(ta, tb)).  A hit iff t_near <= t_far and t_near > 0, at t = t_near (a box behind the origin or containing it never returns).
 *   Ground: for dz < 0, t = (ground_z - oz)/dz, a candidate iff t > 0.  Winner: the smallest t, the lowest box index on equal t, a box over the ground.
 * A ray returns iff r_min <= t <= r_max (closed) and it is not dropped.  The draw: one Philox4x32-10 block per ray, counter (r, sweep, (uint32)step,
 *   0x4C440000 | (step >> 32 & 0xffff)), key seed; word 0: dropped iff uniform24 < p_drop; words 1, 2: nrm = sqrtf(-2 logf(u23)) * cosf(2 pi u23); word 3:
 *   the intensity uniform24 (csrc/lidar_math.h).  t' = fmaf(sigma_r, nrm, (float)t); point = ((float)(t'*dx), (float)(t'*dy), (float)(t'*dz), intensity),
 *   each product in fp64, in the SENSOR frame.  p_drop in [0, 1]; sigma_r finite and >= 0; r_min <= r_max; max_pts > 0.
 * points fp32 [n_sweeps][max_pts][4]: the returns of a sweep in ascending r, the first max_pts kept; n_pts int32 [n_sweeps] = min(returns, max_pts); rows
 *   from n_pts on are zero.  hit int32 [n_sweeps][max_pts] or NULL: 1 + g for box g, 0 for the ground, -1 from n_pts on.  box_hits int32
 *   [n_sweeps][box_cap] or NULL: the KEPT returns of box g.
 * workspace: DEVICE, 8-byte aligned, workspace_bytes >= v2x_lidar_cast_workspace_size (-1 for sizes out of range); it needs no initialisation.
 * n_sweeps == 0: nothing to do (V2X_OK), whatever the other arguments are.
 * v2x_lidar_visible_boxes: box g of sweep s is ground truth iff it is valid, its hits are >= min_hits -- box_hits[s][g], or with any_agent != 0
 *   box_hits[q][g] of any sweep q of the same frame --, its centre in the sensor frame (x, y) = R_s^T (c - o) (fp64, rounded once) has |x| < x_lim and
 *   |y| < y_lim (compared in fp64), and it does not contain the sensor origin (closed slabs, the cast's lx, ly).  gt_boxes fp32 [n_sweeps][box_cap][5]:
 *   rows (x, y, w, h, yaw_g - yaw_s), the yaw difference an fp32 subtraction, not wrapped, in ascending box index, rows past gt_count zero; gt_count
 *   int32 [n_sweeps].  What v2x_det_assign_targets reads. */
long long v2x_lidar_cast_workspace_size(long long n_sweeps, int n_beams, int n_az, int box_cap);
int v2x_lidar_cast(const float *sensors, const int32_t *frame_of, long long n_sweeps, const float *boxes, const int32_t *box_count, int n_frames,
                   int box_cap, const float *beam, int n_beams, const float *az, int n_az, float ground_z, float r_min, float r_max, float sigma_r,
                   float p_drop, uint64_t seed, uint64_t step, float *points, int32_t *n_pts, int max_pts, int32_t *hit, int32_t *box_hits,
                   void *workspace, long long workspace_bytes, v2x_stream_t stream);
int v2x_lidar_visible_boxes(const int32_t *box_hits, const float *sensors, const int32_t *frame_of, long long n_sweeps, const float *boxes,
                            const int32_t *box_count, int n_frames, int box_cap, int min_hits, int any_agent, float x_lim, float y_lim,
                            float *gt_boxes, int32_t *gt_count, v2x_stream_t stream);
/* Moving scenes (DESIGN.md section 3.12 "moving scenes"): the same cast with time.  Every box and every sensor moves in a straight line at constant
 * velocity with a fixed yaw (no turning, no vertical motion); sensors and boxes give the poses at time 0 in the row formats above, frame_of the sweep's
 * world -- many sweeps at different times may share one world.  The same contract: two launches (one for the ground truth), no allocation, no host
 * synchronisation, capturable, every output element written, two calls give identical bytes, n_sweeps == 0 returns V2X_OK before any other check.
 * box_vel fp32 [n_frames][box_cap][2]: world-frame (vx, vy) of each box; sensor_vel fp32 [n_sweeps][2]: world-frame velocity of each sweep's sensor;
 *   time_of fp32 [n_sweeps]: the time at which the sweep starts, seconds; az_time fp32 [n_az]: the time offset of each azimuth step within a sweep (the
 *   host supplies the table, as it supplies every cos / sin pair).
 * The rule, fp64 from the fp32 inputs, every product and sum rounded on its own: ray r = b * n_az + a of sweep s is cast at T = (double)time_of[s] +
 *   (double)az_time[a].  For box g: q = (vsx - vgx, vsy - vgy); lx0 = px*cg + py*sg, ly0 = -px*sg + py*cg with p = o0 - c0 as above; dlx = qx*cg + qy*sg,
 *   dly = -qx*sg + qy*cg; lx = lx0 + dlx*T, ly = ly0 + dly*T.  Everything else is the static rule word for word, evaluated at the ray's own time: w, ux,
 *   uy, the z slab with lz = oz, the slab test, the ground, the winner and its ties, r_min / r_max, the draw on (seed, step, sweep, ray), the range noise;
 *   the point is t' * d in the SENSOR frame at the ray's time (a raw sweep: no ego-motion compensation).  A box whose velocity equals the sensor's has
 *   q = 0 exactly.  With all velocities zero, or all times zero, the outputs are v2x_lidar_cast's bytes.
 * Not finite: a box with a non-finite velocity is dropped, keeping its index.  A sweep whose time_of or sensor_vel is not finite meets no box and has
 *   no ground truth (gt_count 0); a ray whose az_time is not finite meets no box.  The ground does not move and still answers both.
 * workspace: as v2x_lidar_cast's, of v2x_lidar_cast_workspace_size bytes.
 * v2x_lidar_visible_boxes_moving: the ground truth of sweep s at T_ref = (double)time_of[s] + (double)t_ref (t_ref finite; the tools pass half the sweep
 *   duration).  Box g is ground truth iff it is valid (finite velocity included), its hits are >= min_hits -- box_hits[s][g], or with any_agent != 0
 *   box_hits[q][g] of any sweep q of the same world with time_of[q] == time_of[s] (fp32 equality) --, its centre relative to the sensor e = (c0 - o0) +
 *   (vg - vs) * T_ref, rotated into the sensor frame (x, y) = R_s^T e (fp64, every operation rounded, rounded once to fp32 at the end), has |x| < x_lim
 *   and |y| < y_lim, and it does not contain the sensor origin at T_ref (closed slabs, the cast's lx, ly at T = T_ref).  gt_boxes, gt_count as
 *   v2x_lidar_visible_boxes gives them; gt_ids int32 [n_sweeps][box_cap]: the box index of each row -- the car's identity within its world --, -1 past
 *   gt_count; gt_vel fp32 [n_sweeps][box_cap][2] or NULL: vg - vs rotated into the sensor frame (fp64, rounded once), zero past gt_count.  Rows in
 *   ascending box index. */
int v2x_lidar_cast_moving(const float *sensors, const float *sensor_vel, const float *time_of, const int32_t *frame_of, long long n_sweeps,
                          const float *boxes, const float *box_vel, const int32_t *box_count, int n_frames, int box_cap, const float *beam, int n_beams,
                          const float *az, const float *az_time, int n_az, float ground_z, float r_min, float r_max, float sigma_r, float p_drop,
                          uint64_t seed, uint64_t step, float *points, int32_t *n_pts, int max_pts, int32_t *hit, int32_t *box_hits, void *workspace,
                          long long workspace_bytes, v2x_stream_t stream);
int v2x_lidar_visible_boxes_moving(const int32_t *box_hits, const float *sensors, const float *sensor_vel, const float *time_of, float t_ref,
                                   const int32_t *frame_of, long long n_sweeps, const float *boxes, const float *box_vel, const int32_t *box_count,
                                   int n_frames, int box_cap, int min_hits, int any_agent, float x_lim, float y_lim, float *gt_boxes, int32_t *gt_count,
                                   int32_t *gt_ids, float *gt_vel, v2x_stream_t stream);

/* ---------------------------------------------------------------- f-2: visibility maps (upstream's data preparation: `vis_maps`, Config.use_vis)
 * The voxeliser keeps where a sweep's returns end; these entries keep the space each beam crossed before it returned.  The rule -- DESIGN.md section
 * 3.13 -- in short: jobs as in v2x_voxelize_fused_bits (job j moves cloud src_cloud[j] by xform[j], fp32 ((x*m0 + y*m1) + z*m2) + m3 with every
 * operation rounded, and writes into grid dst_grid[j]; several jobs may share a target; a job naming a cloud or grid that does not exist is skipped),
 * plus a ray origin origin[j] (device fp32 [n_jobs][3], in the cloud's frame) moved by the same arithmetic.  origin == NULL: the zero vector (a ray-cast
 * sweep; the moved origin is then the translation column); xform == NULL: identity; src_cloud == dst_grid == NULL (both or neither): job j = cloud j ->
 * grid j.  A moved coordinate c of axis k becomes q = quot(c) - floor(lo_k / voxel_k) in fp64, quot = a1's (the exact reciprocal's product for a
 * power-of-two voxel size, else the division): voxel faces are the integers, the grid is the box [0,X] x [0,Y] x [0,Z].  The segment q_o -> q_p is
 * clipped to the box and walked row by row in x and column by column in y; in each column the ray's z at entry and at exit give a contiguous range of
 * z bits: one OR.  Every crossing parameter is computed from its lattice index, (i - q_o) / d, never accumulated; every fp64 operation is rounded on its
 * own.  Voxels are closed: a ray touching a face, edge or corner sets the voxels on both sides.  A ray is skipped when its index is >= min(n_pts,
 * max_pts), when a moved coordinate is not finite, when it has zero length or when it never meets the box.  An origin outside the grid is legal (the
 * clipped part is walked); an endpoint outside carves to the exit.  The endpoint's own voxel gets no special treatment: occupied is a1's result
 * (v2x_voxelize_bits / v2x_voxelize_fused_bits on the same clouds and jobs), free is trav & ~occ, unknown is neither.  A return in the sliver between
 * the index lattice and a1's open extents is not occupied, so its voxel may read as free.
 * trav_bits: [n_grids][X][Y] uint32, bit z = some ray passed through voxel (x, y, z); cleared by the call, every word written; Z <= 32, n_jobs <= 65535.
 * No allocation, no host synchronisation, capturable; OR is idempotent: the bytes do not depend on the order, two calls give the same.  Two kernel
 * forms, bit-identical, chosen by the grid's shape alone: Z <= 16 with X * Y 16-bit pixels within 128 KiB and X * Y % 8 == 0 (and a 16-byte aligned
 * trav_bits) keeps the grid in LDS, cut into bands of 16 rows, one workgroup per grid and band; any other shape ORs into the cleared grid with
 * device-scope atomics. */
int v2x_lidar_freespace_bits(const float *pts, const int32_t *n_pts, int n_clouds, int max_pts, int pt_stride, const float *origin, const float *xform,
                             const int32_t *src_cloud, const int32_t *dst_grid, int n_jobs, int n_grids, const double *extents, const double *voxel,
                             const int32_t *dims_xyz, uint32_t *trav_bits, v2x_stream_t stream);
/* occ / trav bits -> upstream's vis_maps layout [n][X][Y][Z] fp32: v_occ where occupied, v_free where trav & ~occ, else v_unknown.  Every element is written. */
int v2x_vis_bits_to_dense_f32(const uint32_t *occ_bits, const uint32_t *trav_bits, int n, int X, int Y, int Z, float v_occ, float v_free, float v_unknown,
                              float *out, v2x_stream_t stream);
/* Segmentation labels (uint8 [n][X][Y], v2x_seg_rasterize's) with the cells nobody observed set to the ignore class: labels_out[m][x][y] = ignore where
 * ((occ | trav) & z_mask) == 0, else labels_in.  ignore in [0, 255].  In place (labels_out == labels_in) is allowed: an element is read and written by
 * one thread only. */
int v2x_vis_mask_labels(const uint8_t *labels_in, const uint32_t *occ_bits, const uint32_t *trav_bits, int n, int X, int Y, uint32_t z_mask, int ignore,
                        uint8_t *labels_out, v2x_stream_t stream);

/* ---------------------------------------------------------------- f-1: the metric (coperception/utils/mean_ap.py::eval_map)
 * Upstream intersects shapely polygons on the host; here the IoU of rotated boxes (x, y, w, h, yaw) is a convex clip in
 * fp64 on the device.
 * v2x_rotated_iou: boxes_a fp32 [na][5], boxes_b fp32 [nb][5] -> iou fp32 [na][nb].  Extents w, h >= 0: a rectangle of zero width or
 * height has IoU 0 with everything (itself included); a negative or NaN extent is out of contract (the result is unspecified). */
int v2x_rotated_iou(const float *boxes_a, int na, const float *boxes_b, int nb, float *iou, v2x_stream_t stream);
/* v2x_match_detections: eval_map's per-image matching (mmdet tpfp_default).  det_boxes fp32 [n_img][det_cap][5] in DESCENDING
 * score order (what v2x_det_postprocess emits), det_count int32 [n_img]; gt_boxes fp32 [n_img][gt_cap][5], gt_count int32
 * [n_img] (gt_cap <= 8192).  Each detection takes the ground truth of highest IoU (lowest index on ties) and is a true positive
 * iff IoU >= iou_thr and that box is still free.  tp int32 [n_img][det_cap] (1 / 0; entries >= det_count untouched),
 * best_iou fp32 [n_img][det_cap] or NULL.  AP itself = a sort + two cumulative sums over (score, tp) of all images: the
 * caller's (v2x_sim_amd/utils/postprocess.py::average_precision). */
int v2x_match_detections(const float *det_boxes, const int32_t *det_count, int det_cap, const float *gt_boxes,
                         const int32_t *gt_count, int gt_cap, int n_img, float iou_thr, int32_t *tp, float *best_iou,
                         v2x_stream_t stream);
/* v2x_det_map: the AP table of a whole split -- all maps, all agents (groups), all IoU thresholds -- in ONE call: four launches, no atomics, no
 * allocation, no host synchronisation (capturable), bit-reproducible.  The frozen rule is DESIGN.md section 3.11.
 * INPUT (device): det_boxes fp32 [n_img][det_cap][5] (x, y, w, h, yaw), each map in DESCENDING score order (what v2x_det_postprocess emits);
 *   det_scores fp32 [n_img][det_cap], FINITE (a NaN or infinite score of a counted detection is out of contract); det_count int32 [n_img];
 *   gt_boxes fp32 [n_img][gt_cap][5]; gt_count int32 [n_img]; counts are clamped to [0, cap] as v2x_match_detections does.  group int32 [n_img]:
 *   the agent of each map in [0, n_groups); any other value (-1 by convention: an agent with an empty sweep) keeps the map out of every count and
 *   list -- its scores are never read.  iou_thr fp32 [n_thr] on the DEVICE, each in (0, 1], any order, duplicates allowed.
 * MATCHING: v2x_match_detections' rule and arithmetic (one definition, csrc/det_match.h).  A detection's ground truth is the one of highest rotated
 *   IoU (fp64 clip), lowest index on ties, none at IoU 0 -- found ONCE and shared by all thresholds; the greedy walk in score order keeps one
 *   "taken" set PER THRESHOLD (true positive at t iff IoU >= (double)iou_thr[t] and the ground truth is free at t).
 * RANKING: per group, stable descending by the fp32 score VALUE (-0.0 and +0.0 tie); ties by ascending map index, then ascending position in the
 *   map -- numpy's stable argsort(-scores) over the image-major concatenation.
 * AP: mmdet "area" mode in float64 (v2x_sim_amd/utils/postprocess.py::average_precision): along the ranked list tp_i, fp_i cumulative counts,
 *   recall_i = tp_i / num_gt, precision_i = tp_i / (tp_i + fp_i), envelope = suffix maximum of the precision, area = sum over the positions where
 *   the recall changes of (recall step) x envelope.  num_gt == 0 or no detections: 0.
 * OUTPUT (device; EVERY element is written, the caller clears nothing): ap double [n_groups][n_thr]; num_gt, num_det long long [n_groups];
 *   num_tp long long [n_groups][n_thr]; tp uint8 [n_thr][n_img][det_cap] or NULL (1 / 0; entries >= det_count: 0; a map outside every group is
 *   matched like any other); rank int32 [n_img][det_cap] or NULL (the detection's position in its group's ranked list; -1 beyond the count and
 *   for a map outside every group).
 * Limits: det_cap in [1, 4096], gt_cap in [1, 8192], n_groups in [1, 64], n_thr in [1, 8], n_img * det_cap < 2^31.  workspace: DEVICE,
 *   workspace_bytes >= v2x_det_map_workspace_size (-1 for sizes out of range); it needs no initialisation.  Bad sizes, a NULL required pointer or a
 *   short workspace: V2X_EINVAL with a v2x_last_error() text, nothing launched.  n_img == 0: nothing to do (V2X_OK), whatever the other arguments
 *   are -- nothing is written. */
long long v2x_det_map_workspace_size(long long n_img, int det_cap, int gt_cap, int n_groups, int n_thr);
int v2x_det_map(const float *det_boxes, const float *det_scores, const int32_t *det_count, int det_cap, const float *gt_boxes,
                const int32_t *gt_count, int gt_cap, const int32_t *group, long long n_img, int n_groups, const float *iou_thr, int n_thr,
                double *ap, long long *num_gt, long long *num_det, long long *num_tp, uint8_t *tp, int32_t *rank, void *workspace,
                long long workspace_bytes, v2x_stream_t stream);

/* ---------------------------------------------------------------- f-5: tracking (tools/track: SORT on the detections)
 * v2x_assign_iou: the association step alone on caller-supplied IoU matrices.  iou fp32 [n][cap_r][cap_c] (rows = detections, columns = tracks),
 * n_rows / n_cols int32 [n] (clamped to [0, cap_r] / [0, cap_c]), cap_r, cap_c in [1, 64].  direct != 0 (abewley master): when every row and every
 * column has at most one entry > thr, those entries are the matches; otherwise, and always with direct == 0, the assignment that maximises the summed
 * IoU over min(rows, cols) pairs (shortest augmenting paths in fp64).  A pair with IoU < thr is unmatched; a NaN or infinite entry reads as 0.
 * row_to_col int32 [n][cap_r] = the row's column or -1 (rows >= n_rows: -1).  One wave per matrix, every loop bounded by the capacities. */
int v2x_assign_iou(const float *iou, const int32_t *n_rows, const int32_t *n_cols, int n, int cap_r, int cap_c, float thr, int direct,
                   int32_t *row_to_col, v2x_stream_t stream);
/* v2x_sort_step: one frame of SORT (Kalman constant-velocity box filter, IoU association, births and deaths) for n independent streams in ONE
 * launch, no host round trip (capturable).  Per stream: predict every live track, drop tracks whose predicted box is not finite, associate
 * (v2x_assign_iou's rule), update the matched tracks (Joseph form), one new track per unmatched detection in detection order, report, remove tracks
 * with time_since_update > max_age (stable: storage order = ascending id).
 * det_boxes: box_format 0: fp32 [n][det_cap][4] (x1, y1, x2, y2); 1 / 2: fp32 [n][det_cap][5] (x, y, w, h, yaw) with w (1) / h (2) along the
 *   heading -- the measurement is the stand-up box of the four corners (what v2x_det_postprocess emits; 2 = Config.box_wh_axis "h_along_heading").
 * det_count int32 [n]: only the first 64 detections of a map are read (status bit 0 when there were more); < 0 (the post-processor's "more than
 *   cap candidates" marker): the frame has no detections, status bit 2.
 * STATE, caller-owned; all-zero = the empty tracker (no init entry):
 *   trk_f fp32 [n][t_cap][17]: x[7] = (u, v, s, r, u', v', s') -- centre, area, aspect and their rates --, then the covariance's non-zero pattern
 *         Puu, Puu', Pu'u', Pvv, Pvv', Pv'v', Pss, Pss', Ps's', Prr (with SORT's F, H, Q, R the other entries stay zero);
 *   trk_i int32 [n][t_cap][5]: id, time_since_update, hits, hit_streak, age;
 *   stream_i int32 [n][4]: n_tracks, next_id (the number of ids given so far; ids start at 1 and are never reused), frame_count,
 *         status (sticky bits: 0 detections truncated to 64, 1 births dropped at t_cap, 2 negative det_count).   t_cap in [1, 64].
 * OUTPUT: the tracks with time_since_update == 0 and (hit_streak >= min_hits or frame_count <= min_hits), in ascending id:
 *   out_boxes fp32 [n][t_cap][4] (x1, y1, x2, y2 of the updated state), out_ids int32 [n][t_cap], out_det int32 [n][t_cap] (the index of the
 *   detection the track matched this frame), out_count int32 [n].  Entries >= out_count are not written. */
int v2x_sort_step(const float *det_boxes, const int32_t *det_count, int n, int det_cap, int box_format, float *trk_f, int32_t *trk_i,
                  int32_t *stream_i, int t_cap, float iou_thr, int max_age, int min_hits, int direct, float *out_boxes, int32_t *out_ids,
                  int32_t *out_det, int32_t *out_count, v2x_stream_t stream);
/* v2x_hota_sequences: the HOTA family (TrackEval's hota.py) of n_seq padded sequences in FIVE launches whatever n_seq and
 * n_frames are, no host round trip (capturable), no atomics: the result does not depend on the schedule, and a sequence's rows do not depend on
 * the padding or on the other sequences of the call.
 * gt_boxes fp32 [n_seq][n_frames][cap][4] (x1, y1, x2, y2; 16-byte aligned), gt_ids int32 [n_seq][n_frames][cap], gt_count int32
 *   [n_seq][n_frames] (clamped to [0, cap]); trk_boxes, trk_ids, trk_count the same for the tracks.  cap in [1, 64].  Ids are per sequence and
 *   contiguous, 0 .. n_gt_ids - 1 / 0 .. n_trk_ids - 1 (the largest id spaces of the call); a box whose id lies outside is absent everywhere.
 *   An id twice in one frame is a caller error: unspecified result, memory-safe and terminating.
 * Similarity = the IoU of the axis-aligned boxes in fp64, a NaN or infinite value reads as 0.
 * alpha: DEVICE fp64 [n_alpha], n_alpha in [1, 32]: the thresholds (a matched pair counts for alpha when S >= alpha - 2^-52).
 * workspace: DEVICE, 16-byte aligned, workspace_bytes >= v2x_hota_workspace_size(the same six sizes) (0: sizes out of range or an overflow); it
 *   needs no initialisation and holds nothing the caller needs afterwards.
 * OUTPUT per sequence and alpha: out_i int32 [n_seq][n_alpha][3] = TP, FN, FP; out_f fp64 [n_seq][n_alpha][4] = AssA, AssRe, AssPr and the
 *   sum of the matched similarities (LocA = that sum / TP).  DetA, DetRe, DetPr, HOTA and the combination over sequences follow from these on the
 *   host (v2x_sim_amd/utils/mot_metrics.py::Hota).  n_seq x n_frames and n_seq x n_gt_ids x ceil(n_trk_ids / 64) <= 2^24. */
size_t v2x_hota_workspace_size(int n_seq, int n_frames, int cap, int n_gt_ids, int n_trk_ids, int n_alpha);
int v2x_hota_sequences(const float *gt_boxes, const int32_t *gt_ids, const int32_t *gt_count, const float *trk_boxes, const int32_t *trk_ids,
                       const int32_t *trk_count, int n_seq, int n_frames, int cap, int n_gt_ids, int n_trk_ids, const double *alpha, int n_alpha,
                       void *workspace, size_t workspace_bytes, int32_t *out_i, double *out_f, v2x_stream_t stream);
/* v2x_mot_sequences: the CLEAR MOT family and the Identity family (TrackEval's clear.py and identity.py) of n_seq padded
 * sequences in FIVE launches whatever n_seq and n_frames are, no host round trip (capturable), no atomics: a sequence's outputs are bit-identical
 * alone and in any batch, whatever the padding of frames, boxes and ids.
 * INPUT: v2x_hota_sequences' layout and reading, unchanged -- gt_boxes fp32 [n_seq][n_frames][cap][4] (x1, y1, x2, y2; 16-byte aligned), gt_ids
 *   int32 [n_seq][n_frames][cap], gt_count int32 [n_seq][n_frames] (clamped to [0, cap]); the same for the tracks.  cap in [1, 64].  Ids are per
 *   sequence and contiguous, 0 .. n_gt_ids - 1 / 0 .. n_trk_ids - 1; a box whose id lies outside is absent everywhere.  n_gt_ids and n_trk_ids
 *   in [0, 2048]: the id cap (one workgroup's LDS holds the assignment over a sequence's id space); beyond it the size query returns 0.
 *   An id twice in one frame is a caller error: unspecified result, memory-safe and terminating.
 * Similarity S = the IoU of the axis-aligned boxes in fp64 on the fp32 coordinates, operation by operation; a NaN or infinite value reads as 0.
 * CLEAR, frames in order: a frame without ground truth or without tracks adds its boxes to FN / FP and clears the previous-frame matches.
 *   Otherwise score = 1000 [the ground-truth id's track id in the previous frame's matches == this track id] + S, entries with S < thr - 2^-52
 *   zeroed, the maximum-sum assignment in fp64 (nothing is rounded to fp32), a pair is matched when its score > 0.  TP, FN, FP accumulate;
 *   MOTP_sum = the matched S, added in frame order, then slot order; IDSW counts a matched id whose last matched track id, any frame back,
 *   exists and differs.  Per ground-truth id: present (frames with a valid box, frames without tracks included), matched, starts (matched and
 *   not in the previous frame's matches).  Over the ids with present > 0, in integers: MT = #{5 matched > 4 present}, PT = #{5 matched >=
 *   present} - MT, ML = #{present > 0} - MT - PT, Frag = sum of max(0, starts - 1).  An id that never occurs counts for nothing.
 * IDENTITY: pmc[g][k] = frames in which g and k are both present with S >= thr (plain fp64 comparison, no epsilon); IDTP = the maximum over
 *   partial one-to-one matchings of ids of the summed pmc (an optimal assignment, never a greedy one; the weights are integers, so the value is
 *   unique), IDFN = the ground-truth boxes - IDTP, IDFP = the track boxes - IDTP.
 * thr: finite.  workspace: DEVICE, 16-byte aligned, workspace_bytes >= v2x_mot_workspace_size(the same five sizes) (0: sizes out of range, an
 *   id space beyond the cap or an overflow); it needs no initialisation and holds nothing the caller needs afterwards.
 * OUTPUT per sequence: out_i int32 [n_seq][11] = TP, FN, FP, IDSW, MT, PT, ML, Frag, IDTP, IDFN, IDFP; out_f fp64 [n_seq][1] = MOTP_sum.
 *   MOTA, MOTP, IDF1 ... and the combination over sequences follow on the host (v2x_sim_amd/utils/mot_metrics.py::ClearIdentity).
 *   n_seq x n_frames and n_seq x n_gt_ids x ceil(n_trk_ids / 64) <= 2^24. */
size_t v2x_mot_workspace_size(int n_seq, int n_frames, int cap, int n_gt_ids, int n_trk_ids);
int v2x_mot_sequences(const float *gt_boxes, const int32_t *gt_ids, const int32_t *gt_count, const float *trk_boxes, const int32_t *trk_ids,
                      const int32_t *trk_count, int n_seq, int n_frames, int cap, int n_gt_ids, int n_trk_ids, double thr, void *workspace,
                      size_t workspace_bytes, int32_t *out_i, double *out_f, v2x_stream_t stream);

/* ---------------------------------------------------------------- d: calibration probes (measurement)
 * No upstream counterpart.  The roofline fractions bench.py prints are graded against the datasheet peaks (8 TB/s, 2.5 PFLOP/s bf16);
 * these two probes measure, on the box the bench runs on, what a pure streaming kernel and a pure MFMA loop sustain, so that fractions
 * and rounds can be compared box-free (bench.py: "calibration").
 * v2x_calib_stream: n_read read streams (src, n_read * units * 16 bytes) and n_write write streams (dst, n_write * units * 16 bytes),
 *   16 bytes per lane, fully coalesced; mixes built: 1:1, 1:3 (the det heads), 2:1, 4:1 (conv1_1), 1:0, 0:1.  nontemporal != 0: nt loads /
 *   stores.  wg_per_cu: persistent workgroups of 256 lanes per CU (<= 0: 8).  Bytes moved = (n_read + n_write) * units * 16.
 * v2x_calib_mfma: one 512-lane workgroup per CU, every wave issues iters * 16 independent v_mfma_f32_16x16x32_bf16 (shape32 != 0: iters * 8
 *   v_mfma_f32_32x32x16_bf16) on register operands; seed != 0: random operand bits (the power-limited rate), 0: constants.  *flops (HOST,
 *   may be NULL) = FLOPs of the launch; clocks (DEVICE uint64[2], may be NULL) = shader cycles and 100-MHz ticks elapsed over one wave's loop
 *   (sustained shader clock in MHz = 100 * clocks[0] / clocks[1]).  scratch: DEVICE, >= 512 floats. */
int v2x_calib_stream(const void *src, void *dst, int64_t units, int n_read, int n_write, int nontemporal, int wg_per_cu,
                     v2x_stream_t stream);
int v2x_calib_mfma(float *scratch, int iters, uint32_t seed, int shape32, uint64_t *clocks, double *flops, v2x_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* V2X_AMD_H */
