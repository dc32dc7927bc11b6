/*
 * tomo_hip.h -- C ABI of libtomo_hip.so, the MI355X (gfx950) implementation of the
 * mask stack -> scalar field ("SDF") -> marching-cubes mesh path.
 *
 * The reference (victorramirez952/tomography_3d_reconstructor) has no FFI: its boundary for
 * this path is two Python classes (voxel_processor.py:27-164, surface_extractor.py:28-149)
 * that call NumPy / scipy.ndimage / scikit-image.  This library is what the drop-in classes in
 * tomography_3d_reconstructor_amd/{voxel_processor,surface_extractor}.py bind with ctypes (see
 * INTEGRATION.md); every entry point names the reference line(s) it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer into caller-owned (torch-allocated) memory unless the
 *    parameter name starts with `h_` (host pointer);
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only enqueue work,
 *    they never synchronise, allocate or free (exceptions are stated);
 *  - return value: 0 = ok, negative = TOMO_E_* (never throws across the ABI);
 *  - volume shape is (nz, ny, nx) = (slices, rows, columns); the padded/field shape is
 *    (Nz, Ny, Nx) = (nz + 2p, ny + 2p, nx + 2p) with p = pad in {0, 1};
 *  - "bits" = bit-packed volume: uint64 words, (nz, ny, wx) with wx = tomo_words_per_row(nx);
 *    bit b of word w of a row is voxel x = 64 w + b; bits at x >= nx are zero.
 *
 * Removed in ABI 7 (none had a caller left): tomo_mesh_unique_presorted, tomo_mesh_faces, tomo_mesh_faces_direct, tomo_mesh_faces_workspace_bytes, tomo_mc3_sort_rank, tomo_close_stencil, tomo_pack_close_slab.
 * Removed in ABI 8 (none had a caller left): tomo_morph_pass, tomo_field_signs_fused; tomo_morph_fused accepts nops 2 and 4 only.
 * Removed in ABI 9 (none had a caller left): tomo_close_ends_gp and the separate slab lookup and slab summary entry points
 * (tomo_slab_lookup_summary is both); tomo_mc_scan lost the parameter that had to be NULL.
 */
#ifndef TOMO_HIP_H
#define TOMO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TOMO_OK 0
#define TOMO_E_ARG (-1)       /* bad argument (null pointer, non-positive size, ...) */
#define TOMO_E_LAUNCH (-2)    /* hipGetLastError() after a launch */
#define TOMO_E_SIZE (-3)      /* a count does not fit the index type used */
#define TOMO_E_WORKSPACE (-4) /* workspace too small */

int tomo_abi_version(void);
const char *tomo_error_string(int code);
/* Host-side probe used by the not-gpu tests: evaluates ONE marching-cubes cell with the same
 * code the device runs (compiled for the host).  v = 8 corner values (Lewiner order, float32),
 * tris = up to 36 edge ids (0..12) in LUT order; returns the number of triangles (<0: error). */
int tomo_host_mc_cell(const float *h_v, double iso, int8_t *h_tris, int *h_uses_centre);
double tomo_host_mc_edge_offset(double va, double vb);        /* vertex offset along an edge, same code */
void tomo_host_mc_centre_offset(const double *h_v8, double *h_out3); /* (x,y,z) offset of the centre vertex */

/* Full-content, position-dependent 128-bit checksum of a HOST buffer on `nthreads` host threads (h_out[0..1]).  The
 * device-volume cache of the drop-in classes uses it to make sure a host array the caller could write to still holds
 * what was uploaded (voxel_processor.py:84 / surface_extractor.py:43-46 read the array they are handed). */
int tomo_host_checksum(const void *h_data, int64_t nbytes, int nthreads, uint64_t *h_out);
/* the same with the implementation named (ABI 6): 0 = the fastest the CPU offers (AVX2), 1 = the portable loop; one digest */
int tomo_host_checksum_impl(const void *h_data, int64_t nbytes, int nthreads, int impl, uint64_t *h_out);
/* ... and in two steps (ABI 6), for a buffer that arrives piece by piece (a download in pieces: piece k is digested while piece
 * k + 1 is on the bus): the digests (2 words each) of the tomo_host_checksum_chunk_bytes()-sized chunks of a PART that starts at a
 * chunk boundary, first_chunk = its offset / chunk size; then the fold of all chunk digests of the buffer, in order. */
int64_t tomo_host_checksum_chunk_bytes(void);
int tomo_host_checksum_part(const void *h_part, int64_t nbytes, int64_t first_chunk, int nthreads, int impl, uint64_t *h_dig);
int tomo_host_checksum_fold(const uint64_t *h_dig, int64_t nchunks, int64_t nbytes, uint64_t *h_out);
/* Page a freshly allocated HOST buffer in on `nthreads` threads (one byte per 4 KiB page is written; content unspecified):
 * the 1 B/voxel arrays the drop-in classes hand back (voxel_processor.py:46, :84 create them with np.stack / .copy()) cost
 * ~65 ms per GiB of page faults when a single thread -- or the DMA engine's pinning pass -- touches them first. */
int tomo_host_touch(void *h_data, int64_t nbytes, int nthreads);
/* np.stack (voxel_processor.py:46) on `nthreads` threads: h_dst[i * bytes_each ..] = the bytes_each bytes at h_src[i]. */
int tomo_host_gather(const void *const *h_src, int64_t n, int64_t bytes_each, void *h_dst, int nthreads);
/* SHA-256 with a caller-held, relocatable 112-byte state (ABI 6): the digest of a Z-slab job's WHOLE vertex / face list -- the
 * bytes one np.unique-numbered mesh holds (surface_extractor.py:115-126) -- is formed rank after rank, the state travels
 * between the rank processes instead of the lists.  impl: 0 = fastest available (x86 SHA extensions), 1 = portable code.
 * digest: of everything hashed so far; the state is not changed. */
int tomo_host_sha256_init(void *h_state112);
int tomo_host_sha256_update(void *h_state112, const void *h_data, int64_t nbytes, int impl);
int tomo_host_sha256_digest(const void *h_state112, uint8_t *h_digest32);

/* ---------------------------------------------------------------- geometry helpers (host, pure) */
int64_t tomo_words_per_row(int nx);                      /* ceil(nx / 64) */
/* Extended ("halo") bit volume the field kernel reads: reflect/zero borders materialised. */
int64_t tomo_ext_words_per_row(int nx, int pad);
int64_t tomo_ext_rows(int ny, int pad);                  /* ny + 2 pad + 4 */
int64_t tomo_ext_slices(int nz, int pad);                /* nz + 2 pad + 4 */
/* Field buffer: float32 (Nz, Ny, pitch); padded column X lives at column tomo_field_xorg + X. */
int64_t tomo_field_pitch(int nx, int pad);
int tomo_field_xorg(int pad);                            /* 32 - pad: data column x = 0 sits on a 128-byte line */
int64_t tomo_mc_segments_per_row(int Nx, int xorg);      /* ceil((xorg + Nx + 224) / 256) */

/* ---------------------------------------------------------------- binary stages */
/* np.stack(mask_images) as uint8 0/1 (voxel_processor.py:46) -> bits. */
int tomo_pack_bits(const uint8_t *mask, uint64_t *bits, int nz, int ny, int nx, void *stream);
int tomo_unpack_bits(const uint64_t *bits, uint8_t *mask, int nz, int ny, int nx, void *stream);
/* np.sum(voxel_data) (voxel_processor.py:51): *count (device uint64) += popcount; caller zeroes it. */
int tomo_popcount(const uint64_t *bits, int nz, int ny, int nx, unsigned long long *count, void *stream);
/* ndimage.binary_fill_holes on slice `z` when that slice is non-empty (voxel_processor.py:60-62,66-68).
 * scratch: ny * wx + 8 words.  Iterates on the device until the flood is stable. */
int tomo_fill_holes_slice(uint64_t *bits, int nz, int ny, int nx, int z, uint64_t *scratch, void *stream);
/* The same for slices 0 and nz - 1 in one launch (the two floods are independent); same scratch. */
int tomo_fill_holes_ends(uint64_t *bits, int nz, int ny, int nx, uint64_t *scratch, void *stream);
/* np.stack + _close_volume_ends in one pass over the mask (voxel_processor.py:46, :56-77): the end slices are packed and
 * filled first, then ONE streaming kernel packs every other slice and applies the recurrence, which is the local stencil
 * c'[z] = c[z] | (c[z-1] & c[z+1]).  Needs nz >= 3, nx % 16 == 0 and a 16-byte aligned mask (TOMO_E_ARG otherwise: use
 * tomo_pack_bits + tomo_fill_holes_ends + tomo_close_ends_scan).  scratch: ny * wx + 8 words. */
int tomo_pack_close_ends(const uint8_t *mask, uint64_t *bits, int nz, int ny, int nx, uint64_t *scratch, void *stream);
/* The fused pass for ONE Z-slab of a sharded stack, output slices [z_from, z_to) only: lo_fixed / hi_fixed say that the slab's
 * first / last slice is a GLOBAL end slice, already packed and filled in `bits`; otherwise `below` / `above` (bit-packed
 * (ny, wx) slices with the ORIGINAL content of the neighbour rank's adjacent slice) close the stencil there.  The middle of a
 * slab depends on the mask alone: a Z-slab rank enqueues it before it talks to its neighbours, the end ranges afterwards;
 * `below` / `above` are needed only if the range reaches an end that is not fixed.  Any split of [0, nz) into ranges gives
 * the same bits.  nz >= 2. */
int tomo_pack_close_range(const uint8_t *mask, uint64_t *bits, int nz, int ny, int nx, int z_from, int z_to,
                          const uint64_t *below, const uint64_t *above, int lo_fixed, int hi_fixed, void *stream);
/* Launch-count savers of the Z-slab front (slab.py; scale-out of voxel_processor.py:46, :56-77, no counterpart in the
 * single-process reference): tomo_pack_bits_pair = two tomo_pack_bits in one launch (the original edge slices for the two
 * neighbours; needs nx % 16 == 0 and 16-byte aligned masks); tomo_slab_edges = tomo_pack_close_range(0, edge) +
 * tomo_pack_close_range(nz - edge, nz) + the stencil on the lo_n / hi_n ORIGINAL halo slices of the two neighbours (0: no
 * such neighbour) in ONE launch.  The stencil on n bit-packed slices whose neighbours are given separately:
 * out[i] = mid[i] | (prev & next), prev = i ? mid[i-1] : before, next = i < n-1 ? mid[i+1] : after ((ny, wx) words per slice;
 * out must not overlap mid). */
int tomo_pack_bits_pair(const uint8_t *maskA, uint64_t *bitsA, int nzA, const uint8_t *maskB, uint64_t *bitsB, int nzB,
                        int ny, int nx, void *stream);
int tomo_slab_edges(const uint8_t *mask, uint64_t *bits, int nz, int ny, int nx, int edge, const uint64_t *below,
                    const uint64_t *above, int lo_fixed, int hi_fixed, const uint64_t *lo_before, const uint64_t *lo_mid,
                    const uint64_t *lo_after, int lo_n, uint64_t *lo_out, const uint64_t *hi_before, const uint64_t *hi_mid,
                    const uint64_t *hi_after, int hi_n, uint64_t *hi_out, void *stream);
/* The z recurrence of _close_volume_ends (voxel_processor.py:72-75), in place.
 * workspace: tomo_close_ends_workspace_words() uint64 words. */
int64_t tomo_close_ends_workspace_words(int nz, int ny, int nx);
int tomo_close_ends_scan(uint64_t *bits, int nz, int ny, int nx, uint64_t *workspace, void *stream);
/* nops (2 or 4; anything else is TOMO_E_ARG) 6-neighbour passes (skimage binary_erosion / binary_dilation,
 * voxel_processor.py:88,91) fused into one kernel, in != out: bit j of `ops` is the op of pass j, 0 = erosion with
 * border_value 1, 1 = dilation with border value 0.  The masks tomo_smooth plans (E D | D E = ops 0b0110 with nops 4,
 * D E = 0b01 and E D = 0b10 with nops 2) run in kernels compiled for them; a mask tomo_smooth does not plan takes
 * the run-time-mask kernel. */
int tomo_morph_fused(const uint64_t *in, uint64_t *out, int nz, int ny, int nx, uint32_t ops, int nops, void *stream);
/* smooth_voxel_data (voxel_processor.py:79-97) whole, in ONE launch into `out` (in != out): the opening if
 * create_manifold, then ONE closing if iterations >= 1 -- with the reference's border values (dilation pads with 0,
 * erosion with 1) a closing is idempotent, so `iterations` closings leave the bits of one.  No pass at all copies. */
int tomo_smooth(const uint64_t *in, uint64_t *out, int nz, int ny, int nx, int iterations, int create_manifold, void *stream);

/* ---------------------------------------------------------------- callers either side of the path */
/* volume_calculator.py:23-35: counts[z] (device uint64[nz]) = np.sum(voxel_data[z]); the call zeroes counts first. */
int tomo_slice_popcounts(const uint64_t *bits, int nz, int ny, int nx, unsigned long long *counts, void *stream);
/* volume_calculator.py:40,62 (np.where(voxel_data) + min/max): box (device int32[6]) = {zmin, zmax, ymin, ymax, xmin,
 * xmax} of the set voxels; an empty volume gives {INT32_MAX, -1, INT32_MAX, -1, INT32_MAX, -1}. */
int tomo_bbox(const uint64_t *bits, int nz, int ny, int nx, int32_t *box, void *stream);
/* voxel_processor.py:99-127 (np.where(voxel_data), every k-th entry, one float64 row per kept entry) on the resident bits.
 * The RANK g of a set voxel is the number of set voxels in front of it in C order (z, y, x) = word order, then ascending
 * bit; it is kept iff g % k == 0 and becomes row g / k = (z_mm[z], (double)y * mm_y, (double)x * mm_x).
 *   tomo_point_cloud_blocks  number of fixed-size tiles of words the two passes work in
 *   tomo_point_cloud_count   blk_off[i] = rank_base + the set voxels of the tiles before tile i, i <= blocks (a popcount per
 *                            tile, then one single-workgroup 64-bit scan): blk_off[blocks] - rank_base set voxels in all
 *   tomo_point_cloud_rows    row g / k of every kept voxel goes to out + 3 * (g / k - row_first) iff row_first <= g / k <
 *                            row_first + cap_rows; nothing else of `out` is written.  A caller fetches a large cloud in windows
 *                            this way; a Z-slab rank passes rank_base = the set voxels of the ranks below it and row_first =
 *                            ceil(rank_base / k), and its rows are its run of the whole stack's array.  k >= 1; cap_rows = 0
 *                            writes nothing (out may be NULL then).  TOMO_E_SIZE from 2^31 words on. */
int64_t tomo_point_cloud_blocks(int nz, int ny, int nx);
int tomo_point_cloud_count(const uint64_t *bits, int nz, int ny, int nx, uint64_t rank_base, uint64_t *blk_off, void *stream);
int tomo_point_cloud_rows(const uint64_t *bits, int nz, int ny, int nx, const uint64_t *blk_off, int64_t k, const double *z_mm,
                          double mm_y, double mm_x, int64_t row_first, int64_t cap_rows, double *out, void *stream);
/* Connected components of the resident bits (no counterpart in the reference; the semantics are scipy.ndimage.label's with
 * generate_binary_structure(3, 1) -- connectivity 6, the 3-D cross of voxel_processor.py:88,91 -- or (3, 3) -- connectivity 26;
 * anything else is TOMO_E_ARG).  The unit is the X-RUN, a maximal run of set bits in a row; run ids ascend in raster order,
 * the root of a component is its smallest run id, and components are numbered 1..n in the raster order of their first voxel:
 * the output is unique, whatever the schedule.  Working memory scales with the rows and the runs, never with the voxels.
 *   tomo_cc_scan_blocks  uint64 words of the scratch `blk` for a table of n entries
 *   tomo_cc_count_runs   row_off uint32[nz * ny + 1] = runs in front of every row (exclusive scan; the last entry = all runs);
 *                        zeroes tot (device uint64[8]) and sets tot[0] = runs, bit 0 of tot[2] from 2^31 runs on.
 *                        blk: tomo_cc_scan_blocks(nz * ny + 1) words
 *   tomo_cc_label_runs   parent uint32[cap_runs] = the root of every run, rank uint32[cap_runs] = at a root, the number of roots
 *                        in front of it: the label of run r is rank[parent[r]] + 1; tot[1] = n; sizes int64[cap_runs], of which
 *                        the first n = voxels of component 1..n (integer atomics: the same on every run).
 *                        blk: tomo_cc_scan_blocks(cap_runs) words.  The caller reads tot[0] once and passes cap_runs >= it; the
 *                        kernels take the count from tot and touch nothing (bit 1 of tot[2]) if it exceeds cap_runs; a run id
 *                        outside the tables (the bits changed since tomo_cc_count_runs) sets bit 2 and is skipped
 *   tomo_cc_expand       labels int32 (nz, ny, nx): scipy's array
 *   tomo_cc_filter       out (!= bits) = the bits of the components with sizes >= min_voxels; largest: of those only the largest
 *                        one, the lowest label among equals (its label goes to tot[3], 0: none).  Tail bits of out are zero.
 * TOMO_E_SIZE from 2^31 words or cap_runs on. */
int64_t tomo_cc_scan_blocks(int64_t n);
int tomo_cc_count_runs(const uint64_t *bits, int nz, int ny, int nx, uint32_t *row_off, uint64_t *blk, unsigned long long *tot,
                       void *stream);
int tomo_cc_label_runs(const uint64_t *bits, int nz, int ny, int nx, int connectivity, const uint32_t *row_off, int64_t cap_runs,
                       uint32_t *parent, uint32_t *rank, int64_t *sizes, uint64_t *blk, unsigned long long *tot, void *stream);
int tomo_cc_expand(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                   const uint32_t *rank, unsigned long long *tot, int32_t *labels, void *stream);
int tomo_cc_filter(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                   const uint32_t *rank, const int64_t *sizes, unsigned long long *tot, int64_t min_voxels, int largest,
                   uint64_t *out, void *stream);
/* Measurements per component of a labelled volume (the run tables of tomo_cc_label_runs; no counterpart in the reference,
 * whose calculate_voxel_volume_variable_depth / calculate_bounding_box_variable_depth would have to be called on the mask
 * `labels == c` once per component).  One more pass over the runs, integer atomics only: the same on every run.
 *   tomo_cc_measure        table int64[cap][10], row c = component c + 1 for c < n = tot[1]: [0] voxels, [1, 2] zmin, zmax,
 *                          [3, 4] ymin, ymax, [5, 6] xmin, xmax (inclusive indices), [7] sum of z over the voxels, [8] sum of y,
 *                          [9] sum of x (a run [s, e) adds (e - s) * (s + e - 1) / 2, exact).  An init launch writes every
 *                          row first (minima: the largest int64, everything else 0), so rows n .. cap - 1 hold that.  n > cap:
 *                          bit 1 of tot[2] and nothing is measured; a run id outside the tables: bit 2, as above
 *   tomo_cc_zhist_offsets  the keep rule of tomo_cc_filter on column 0 (largest: the label goes to tot[3]): sel uint8[cap], the
 *                          first n = 1 for a selected component; off uint64[cap + 1], the first n + 1 = the exclusive scan
 *                          (64-bit) of zmax - zmin + 1 over the selected ones, 0 for the others; off[n] = tot[4] = the sum,
 *                          which sizes `hist`; slot uint32[cap], the first n = selected components in front of c; tot[5] =
 *                          selected components.  cap = rows of the table >= n (else bit 1 of tot[2], nothing is written);
 *                          blk: 2 * tomo_cc_scan_blocks(cap) words
 *   tomo_cc_select         tomo_cc_zhist_offsets with the whole keep rule: min_voxels <= voxels <= max_voxels (INT64_MAX: no upper
 *                          bound) and, with enclosed != 0, only a component whose inclusive index box touches no face of the
 *                          stack nz, ny, nx (zmin > 0, zmax < nz - 1, likewise y and x; read only then): on the tables of a
 *                          complement, its cavities.  The same outputs, counter words and scratch; tomo_cc_zhist_offsets is this
 *                          call without an upper bound and without the face test.  largest with enclosed or a finite max_voxels:
 *                          TOMO_E_ARG, like max_voxels < 0
 *   tomo_cc_zhist          hist uint64[hist_cap], zeroed here: hist[off[c] + z - zmin[c]] = voxels of selected component c + 1
 *                          in slice z.  tot[4] > hist_cap: bit 1 of tot[2] and nothing is added; a slice outside the
 *                          component's box (the bits changed): bit 2
 *   tomo_cc_zsums          one thread per selected component, its slices in ascending z, w / zc = device float64[nz]:
 *                          vol += (double)count * w[z], mz += ((double)count * w[z]) * zc[z], sequential, never contracted;
 *                          out float64[cap_sel][2] row slot[c] = (vol, mz), labels int64[cap_sel] entry slot[c] = c + 1.
 *                          With w[z] = (mm_x * mm_y) * depth[z], vol is bit for bit volume_calculator.py:23-35 on the mask
 *                          `labels == c`.  tot[4] > hist_cap or tot[5] > cap_sel: bit 1 of tot[2], nothing is written
 * TOMO_E_ARG for a null pointer, a non-positive size or min_voxels < 0; TOMO_E_SIZE from 2^31 words, runs, components or
 * selected components on (2^60 histogram entries). */
int tomo_cc_measure(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                    const uint32_t *rank, unsigned long long *tot, int64_t *table, int64_t cap, void *stream);
int tomo_cc_zhist_offsets(const int64_t *table, int64_t cap, unsigned long long *tot, int64_t min_voxels, int largest, uint8_t *sel,
                          uint64_t *off, uint32_t *slot, uint64_t *blk, void *stream);
int tomo_cc_select(const int64_t *table, int64_t cap, unsigned long long *tot, int64_t min_voxels, int64_t max_voxels, int largest,
                   int enclosed, int nz, int ny, int nx, uint8_t *sel, uint64_t *off, uint32_t *slot, uint64_t *blk, void *stream);
int tomo_cc_zhist(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                  const uint32_t *rank, unsigned long long *tot, const int64_t *table, int64_t cap, const uint8_t *sel,
                  const uint64_t *off, uint64_t *hist, int64_t hist_cap, void *stream);
int tomo_cc_zsums(const int64_t *table, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint64_t *off,
                  const uint32_t *slot, const uint64_t *hist, int64_t hist_cap, const double *w, const double *zc, int nz,
                  double *out, int64_t *labels, int64_t cap_sel, void *stream);
/* Second moments and principal axes per component (no counterpart in the reference).  A set voxel (k, j, i) of component c is a
 * point mass at p = (zc[k], j * mm_y, i * mm_x) -- the coordinates of the distance transform -- of weight w[k] = (mm_x * mm_y) *
 * depth[k], the voxel's volume (the table tomo_cc_zsums gets).  W = sum w; centre = sum w p / W; covariance = sum w (p - centre)
 * (p - centre)^T / W, symmetric 3 x 3 in (z, y, x) order.  Voxels are points: no d^2 / 12 for a voxel's own extent, a plate one
 * voxel thick has variance 0 across itself.  Principal variances = the eigenvalues, descending; principal axes = the unit
 * eigenvectors in that order, the component of largest magnitude positive (the first such on a tie); a zero matrix (one voxel)
 * has variances 0 and the identity.  Tables and selection (sel, off, slot, tot[4], tot[5]) are tomo_cc_zhist_offsets'.
 *   tomo_cc_moment_hist  mom uint64[6 * hist_cap], zeroed here: mom[6 * (off[c] + z - zmin[c]) + 0 .. 5] = over the voxels of
 *                        selected component c + 1 in slice z: their number, sum j', sum i', sum j'^2, sum i'^2, sum j' i' with
 *                        j' = j - ymin[c], i' = i - xmin[c] (the box of tomo_cc_measure).  One pass over the runs, closed forms
 *                        in 64-bit integers, integer atomics only: the same on every run.  tot[4] > hist_cap: bit 1 of tot[2]
 *                        and nothing is added; a slice outside the component's box or a voxel in front of its corner (the bits
 *                        changed): bit 2.  TOMO_E_SIZE where ny * nx * max(ny, nx)^2 >= 2^63: a slice's sum could leave 63 bits
 *   tomo_cc_moments      one thread per selected component, its slices in ascending z twice, w / zc = device float64[nz],
 *                        sequential float64, never contracted.  First walk: W by tomo_cc_zsums' very additions (bit for bit its
 *                        vol), the z moment likewise (centre z = mz / W as there), the first moments about the box corner.
 *                        Second walk: the six central sums about that centre.  Then a cyclic Jacobi iteration (at most 32
 *                        sweeps), the sort, the sign rule.  out float64[cap_sel][22] row slot[c] = W, centre z y x in mm,
 *                        covariance zz zy zx yy yx xx in mm^2, variances (3, clamped at 0), axes (3 rows of 3); labels
 *                        int64[cap_sel] entry slot[c] = c + 1.  tot[4] > hist_cap or tot[5] > cap_sel: bit 1 of tot[2], nothing
 *                        is written; a component without a voxel in its segment: bit 2
 * TOMO_E_ARG for a null pointer, a non-positive size or spacing; TOMO_E_SIZE from 2^31 words, runs, components or selected
 * components on (2^60 / 6 histogram entries). */
int tomo_cc_moment_hist(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                        const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const int64_t *table, int64_t cap,
                        const uint8_t *sel, const uint64_t *off, uint64_t *mom, int64_t hist_cap, void *stream);
int tomo_cc_moments(const int64_t *table, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint64_t *off,
                    const uint32_t *slot, const uint64_t *mom, int64_t hist_cap, const double *w, const double *zc, int nz,
                    double mm_y, double mm_x, double *out, int64_t *labels, int64_t cap_sel, void *stream);
/* Euler number, cavities and handles per component (no counterpart in the reference).  Foreground connectivity k = 6 or 26, the
 * background has the complementary k' = 32 - k, everything outside the stack is background.  chi under 26: V - E + F - C of the
 * union of the closed unit cubes of the set voxels; under 6: N0 - N1 + N2 - N3 of the dual complex (voxels, face-adjacent pairs,
 * 2 x 2 blocks, 2 x 2 x 2 blocks, all set).  Every cell is counted by one voxel (6: its low corner; 26: the raster-first set voxel
 * incident to it), so the voxels of a component add up to the chi of the mask `labels == c`.  cavities = the components of the
 * mask's complement under k' that do not reach the outside; handles = 1 - chi + cavities.  Integer atomics only: the same on
 * every run.
 *   tomo_cc_euler          euler int64[cap], zeroed here: euler[c] = chi of component c + 1 for c < n = tot[1], one pass over the
 *                          rows with word-wide ANDs / ORs and popcounts under the masks of the runs.  parent == NULL: no table is
 *                          read (row_off, rank and tot may be NULL) and euler[0] = chi of the whole volume.  n > cap: bit 1 of
 *                          tot[2] and nothing is added; a run id outside the tables: bit 2
 *   tomo_cc_complement     out (!= bits) = ~bits inside the stack, the bits at x >= nx clear: the background as a bit volume
 *   tomo_cc_cavities       bg_* = the run tables, counters and measurement table (tomo_cc_measure, bg_cap rows) of the complement
 *                          labelled under k'; bg_cap_runs = 0: the volume is full, no bg_* is read.  A background component
 *                          whose box touches no face of the stack is a cavity of the component that holds the voxel left of the
 *                          cavity's first run.  topo int64[cap][3], every row written: (euler[c], cavities, handles) for c < n,
 *                          zeros behind.  A table that does not fit its counters: bit 1 of tot[2]; a left neighbour that is clear
 *                          or outside the tables: bit 2.  bg_tot is only read
 *   tomo_cc_cavity_owners  the argument head of tomo_cc_cavities (through bg_cap), the same owner search: owner int64[bg_cap], every
 *                          entry written, entry c = the label (1-based) of the component that owns background component c + 1
 *                          where that is a cavity, 0 where it reaches a face and behind the bg_tot[1] components.  An island
 *                          floating in a void does not own it.  The guards are tomo_cc_cavities', in tot[2].  bg_cap_runs = 0:
 *                          nothing is written (owner may be NULL)
 *   tomo_cc_topology_rows  out int64[cap_sel][5] row slot[c] = (c + 1, voxels, euler, cavities, handles) for the components
 *                          tomo_cc_zhist_offsets selected (sel, slot, tot[5]); tot[5] > cap_sel: bit 1 of tot[2], nothing is written
 * TOMO_E_ARG for a null pointer, a non-positive size or a connectivity other than 6 / 26; TOMO_E_SIZE from 2^31 words, runs or
 * components on. */
int tomo_cc_euler(const uint64_t *bits, int nz, int ny, int nx, int connectivity, const uint32_t *row_off, int64_t cap_runs,
                  const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, int64_t *euler, int64_t cap, void *stream);
int tomo_cc_complement(const uint64_t *bits, int nz, int ny, int nx, uint64_t *out, void *stream);
int tomo_cc_cavities(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                     const uint32_t *rank, unsigned long long *tot, int64_t cap, const uint64_t *bg_bits, const uint32_t *bg_row_off,
                     int64_t bg_cap_runs, const uint32_t *bg_parent, const uint32_t *bg_rank, const unsigned long long *bg_tot,
                     const int64_t *bg_table, int64_t bg_cap, const int64_t *euler, int64_t *topo, void *stream);
int tomo_cc_cavity_owners(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                          const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, int64_t cap, const uint64_t *bg_bits,
                          const uint32_t *bg_row_off, int64_t bg_cap_runs, const uint32_t *bg_parent, const uint32_t *bg_rank,
                          const unsigned long long *bg_tot, const int64_t *bg_table, int64_t bg_cap, int64_t *owner, void *stream);
int tomo_cc_topology_rows(const int64_t *table, const int64_t *topo, int64_t cap, unsigned long long *tot, const uint8_t *sel,
                          const uint32_t *slot, int64_t *out, int64_t cap_sel, void *stream);
/* Surface area per component by the discretised Crofton formula (Ohser & Muecklich; no counterpart in the reference, whose
 * calculate_surface_area needs a mesh of the whole volume).  Coordinates, spacing and background are the distance transform's:
 * pixel sizes mm_x, mm_y, slice depths d[k], everything outside the stack is background, the virtual slices -1 and nz have the
 * depth of the edge slice next to them.
 * Counts: for a set voxel p of slice k and each of its 26 neighbours q that is clear or outside the stack, one count in
 * n[k][c], for the component of p (no labelling: for the volume as a whole).  The column c follows (|dz|, |dy|, |dx|) of q - p
 * and the sign of dz:   0, 1, 2 = x, y, xy in the slice (2, 2, 4 neighbours);   3, 4, 5, 6 = z, xz, yz, xyz towards slice k + 1
 * (1, 2, 2, 4);   7, 8, 9, 10 = the same towards slice k - 1.  A neighbour that is set but belongs to another component
 * (diagonal contact under connectivity 6) is no transition: under both connectivities the counts of all components add up
 * exactly to the counts of the unlabelled volume.
 * Factors: the lattice height h = d[k] for c < 3, (d[k] + d[k + 1]) / 2 for c = 3 .. 6, (d[k - 1] + d[k]) / 2 for c = 7 .. 10.
 * With (a_z, a_y, a_x) the class of column c and L = sqrt((a_z h)^2 + (a_y mm_y)^2 + (a_x mm_x)^2):
 *     F[k][c] = 2 * w_c(mm_x, mm_y, h) * (mm_x * mm_y * h) / L
 * directions = 13: w_c is twice the fraction of the unit sphere that is closer to (a_z h, a_y mm_y, a_x mm_x) / L than to any
 * other of the 26 normalised lattice directions of the box (h, mm_y, mm_x); the weights of the 13 directions sum to 1 (cubic
 * lattice: 0.09155578240952 for the axes, 0.07396125575216 for the face diagonals, 0.07039127956464 for the cube diagonals).
 * directions = 3: w = 1 / 3 for x, y and z, 0 otherwise.  The host computes F (pipeline.surface_factors).
 * Sum: S = sum over k ascending over the slices of the component's box, over c = 0 .. 10, of (double)n[k][c] * F[k][c]:
 * sequential float64, never contracted (tomo_cc_zsums' discipline).  An axis-aligned flat face is underestimated (an 8^3
 * cube reads 0.8615 of its 384): the known bias of the 13-direction estimator.
 *   tomo_cc_surface_hist  surf uint64[11 * hist_cap], zeroed here: surf[11 * (off[c] + z - zmin[c]) + 0 .. 10] = n[z][0 .. 10] of
 *                         selected component c + 1 (tables and selection: tomo_cc_zhist_offsets').  One thread per row slides
 *                         the row and its eight neighbour rows along x, popcounts under the masks of the runs; integer atomics
 *                         only: the same on every run.  tot[4] > hist_cap: bit 1 of tot[2] and nothing is added; a slice outside
 *                         the component's box or a run id outside the tables: bit 2.  parent == NULL: no table is read (row_off,
 *                         rank, tot, table, sel and off may be NULL), the volume is one component with the box 0 .. nz - 1 at
 *                         entry 0: surf[11 * z + c] = n[z][c]; hist_cap < nz is TOMO_E_ARG then
 *   tomo_cc_surface       one thread per selected component, its slices in ascending z: F = device float64[nz][11]; out
 *                         float64[cap_sel] entry slot[c] = S; counts int64[cap_sel][7] row slot[c] = the counters summed over the
 *                         slices with up and down folded: x, y, xy, z, xz, yz, xyz; labels int64[cap_sel] entry slot[c] = c + 1.
 *                         directions = 3 leaves the columns whose factor is 0 out of the sum (the same S).  tot[4] > hist_cap or
 *                         tot[5] > cap_sel: bit 1 of tot[2], nothing is written.  table == NULL: the unlabelled form (tot, sel, off
 *                         and slot may be NULL), row 0 alone is written, from the entries 0 .. nz - 1, labels[0] = 1
 * TOMO_E_ARG for a null pointer, a non-positive size or directions other than 3 / 13; TOMO_E_SIZE from 2^31 words, runs,
 * components or selected components on (2^60 / 11 histogram entries). */
int tomo_cc_surface_hist(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                         const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const int64_t *table, int64_t cap,
                         const uint8_t *sel, const uint64_t *off, uint64_t *surf, int64_t hist_cap, void *stream);
int tomo_cc_surface(const int64_t *table, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint64_t *off,
                    const uint32_t *slot, const uint64_t *surf, int64_t hist_cap, const double *F, int nz, int directions,
                    double *out, int64_t *counts, int64_t *labels, int64_t cap_sel, void *stream);
/* Mean breadth per component by the discretised Crofton formula (Ohser & Muecklich; no counterpart in the reference): the
 * fourth Minkowski functional, M = 2 pi * mean breadth being the integral of mean curvature.  Lattice and background are the
 * distance transform's: voxel (k, j, i) sits at (zc[k], j mm_y, i mm_x), everything outside the stack is clear.
 *     b = sum over m of c_m * delta_m * chi_m
 * over the 13 families of lattice planes with Miller index m = (a_z, a_y, a_x) in {-1, 0, 1}^3, first non-zero entry positive,
 * in ascending tuple order:
 *     (0,0,1) (0,1,-1) (0,1,0) (0,1,1) (1,-1,-1) (1,-1,0) (1,-1,1) (1,0,-1) (1,0,0) (1,0,1) (1,1,-1) (1,1,0) (1,1,1)
 * For a lattice of height h the normal is n = (a_z / h, a_y / mm_y, a_x / mm_x) (the reciprocal-lattice vector, not the lattice
 * diagonal), the plane spacing delta_m = 1 / |n|, and c_m twice the share of the unit sphere in the Voronoi cell of +-n / |n|
 * among the 26 such normals (the weights of tomo_cc_surface on the reciprocal box (1 / h, 1 / mm_y, 1 / mm_x); over the 13
 * families they sum to 1).  directions = 3: the three axis normals with c = 1 / 3 each.
 * chi_m is the sum over all planes a . p = const of the 2-D Euler number V - E + F of the section, on the lattice of the plane:
 *   one non-zero entry (3 families)    edges: the two other axis steps; faces: the unit squares they span
 *   two (6 families)                   edges: the axis step u of the zero entry and the one face diagonal e perpendicular to m;
 *                                      faces: the rectangles (p, p + u, p + e, p + u + e)
 *   three (4 families)                 edges: the three face diagonals perpendicular to m (a triangular lattice, e2 = e1 + e3);
 *                                      faces: the triangles (p, p + e1, p + e2) and (p, p + e3, p + e2)
 * An edge counts when both its ends are set, a face when all its corners are.  Every step is a 26-neighbour offset.
 * Every cell is anchored at its raster-first corner p: filed in the slice of p and credited to the component of p.  Under
 * connectivity 26 all corners of a cell lie in one component and a row is exactly the value of the mask `labels == c`; a cell
 * across a diagonal contact under connectivity 6 goes to the component of its first corner: under both connectivities the
 * counts of all components add up exactly to the counts of the unlabelled volume.  All cells of p lie in its forward
 * neighbourhood: its own row at x + 1, row (z, y + 1) at x - 1 .. x + 1, rows (z + 1, y - 1 .. y + 1) at x - 1 .. x + 1.
 * Depths: a cell whose corners all lie in slice k (every vertex is one) is IN the slice and uses h = d[k]; a CROSS cell has
 * corners in slices k and k + 1 and uses h = (d[k] + d[k + 1]) / 2.  No cell leaves the stack.  B = float64[nz][26]
 * (pipeline.breadth_factors): columns 0 .. 12 c_m delta_m at d[k], 13 .. 25 at the mean depth; the cross columns are 0.0 in the
 * last slice, and that of (1, 0, 0), which has no cross cell, everywhere.
 * Sum: b = sum over k ascending over the slices of the component's box, over the columns 0 .. 25, of
 * (double)(int64)chi[k][column] * B[k][column], chi^in in the columns 0 .. 12 and chi^cross in 13 .. 25: sequential float64,
 * never contracted (tomo_cc_zsums' discipline).  directions = 3: only the columns of (0,0,1), (0,1,0) and (1,0,0) enter.
 *   tomo_cc_breadth_hist  hist uint64[18 * hist_cap], zeroed here; arguments, selection and guard bits are
 *                         tomo_cc_surface_hist's.  Entry off[c] + z - zmin[c] holds, for the cells anchored in slice z of
 *                         component c + 1: words 0 .. 5 the raw counts inside the slice -- voxels, edges along x, along y, along
 *                         (0, 1, 1), along (0, 1, -1), squares x y -- and words 6 .. 17 the signed chi^cross (faces - edges, two's
 *                         complement) of the families in the order above without (1, 0, 0).  One thread per row slides the row
 *                         and four forward rows along x; word-wide ANDs, popcounts under the masks of the runs, wrapping integer
 *                         atomics only: the same bytes on every run.  parent == NULL: the volume is one component, entry z.
 *   tomo_cc_breadth       one thread per selected component: chi^in = voxels - edges (+ squares for (1, 0, 0)) from the raw
 *                         counts; out float64[cap_sel] entry slot[c] = b; section_euler int64[cap_sel][13] row slot[c] = chi^in +
 *                         chi^cross summed over the slices; labels int64[cap_sel] entry slot[c] = c + 1.  Guards and the
 *                         unlabelled form (table == NULL: row 0 from the entries 0 .. nz - 1) are tomo_cc_surface's.
 * TOMO_E_ARG for a null pointer, a non-positive size or directions other than 3 / 13; TOMO_E_SIZE from 2^31 words, runs,
 * components or selected components on (2^60 / 18 histogram entries). */
int tomo_cc_breadth_hist(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                         const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const int64_t *table, int64_t cap,
                         const uint8_t *sel, const uint64_t *off, uint64_t *hist, int64_t hist_cap, void *stream);
int tomo_cc_breadth(const int64_t *table, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint64_t *off,
                    const uint32_t *slot, const uint64_t *hist, int64_t hist_cap, const double *B, int nz, int directions,
                    double *out, int64_t *section_euler, int64_t *labels, int64_t cap_sel, void *stream);
/* Inscribed sphere and local thickness per component (no counterpart in the reference).  Distance and local thickness are local
 * to a component: the nearest site of a voxel of component A is never a voxel of another component (stepping from such a site
 * towards the voxel ends at an unset voxel that is no farther), and the open digital ball round a centre where it fits is
 * 6-connected through set voxels.  So D2 of the whole volume equals D2 of the mask `labels == c` under that mask, bit for bit,
 * and so does the level map; ONE transform serves every component -- and every cavity, on the tables of the complement -- and
 * what is left is a reduction of a per-voxel value over the run tables.  One wave per 64-bit word of a row, one lane per bit: the
 * per-voxel array is read in whole rows; the runs of the word and their components are wave-uniform.  The value of a set voxel
 * is v = (float)sqrt(d2): read from dist, the float32 map of tomo_edt_distance, or formed from d2, the float64 map of
 * tomo_edt_squared -- the same bits; exactly one of the two is not NULL.  Integer min / max / add atomics only: the same bytes
 * on every run.
 *   tomo_cc_value_max    best uint32[cap], zeroed here: best[c] = the largest float32 bit pattern of v over component c + 1 (v >=
 *                        0: unsigned order is float order); per run of a word one wave maximum and one atomicMax
 *   tomo_cc_value_first  after tomo_cc_value_max, on the same arrays: first uint64[cap], set to all ones here: first[c] = the
 *                        smallest flat index (z * ny + y) * nx + x whose v has the bits best[c]; per run one 64-bit atomicMin
 *   tomo_cc_value_rows   out int64[cap_sel][4] row slot[c] = (c + 1, voxels, best[c], first[c]) for the components tomo_cc_select
 *                        selected (sel, slot, tot[5]); tot[5] > cap_sel: bit 1 of tot[2], nothing is written
 *   tomo_cc_level_hist   hist uint64[(levels + 1) * hist_cap], zeroed here: hist[(levels + 1) * (off[c] + z - zmin[c]) + l] = the
 *                        voxels of selected component c + 1 in slice z whose entry of level, the int32 (nz, ny, nx) level map of
 *                        the local thickness (tomo_edt_cover), is l; an entry outside 0 .. levels counts as 0.  Inside a run the
 *                        lanes of one level add once.  tot[4] > hist_cap: bit 1 of tot[2] and nothing is added; a slice outside
 *                        the component's box or a run id outside the tables: bit 2
 *   tomo_cc_level_sums   per selected component and level l its slices in ascending z, w = device float64[nz]: voxels
 *                        int64[cap_sel][levels + 1] row slot[c] = the counts summed; volume float64[cap_sel][levels] entry l - 1
 *                        = acc, acc = acc + (double)count * w[z], sequential float64, never contracted (tomo_cc_zsums'
 *                        discipline); labels int64[cap_sel] entry slot[c] = c + 1.  tot[4] > hist_cap or tot[5] > cap_sel: bit 1
 *                        of tot[2], nothing is written
 * TOMO_E_ARG for a null pointer, a non-positive size, levels < 0, both or neither of dist and d2; TOMO_E_SIZE from 2^31 words,
 * runs, components or selected components on (2^60 / (levels + 1) histogram entries). */
int tomo_cc_value_max(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                      const uint32_t *rank, unsigned long long *tot, const float *dist, const double *d2, uint32_t *best,
                      int64_t cap, void *stream);
int tomo_cc_value_first(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                        const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const float *dist, const double *d2,
                        const uint32_t *best, uint64_t *first, int64_t cap, void *stream);
int tomo_cc_value_rows(const int64_t *table, const uint32_t *best, const uint64_t *first, int64_t cap, unsigned long long *tot,
                       const uint8_t *sel, const uint32_t *slot, int64_t *out, int64_t cap_sel, void *stream);
int tomo_cc_level_hist(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                       const uint32_t *rank, unsigned long long *tot, const int64_t *table, int64_t cap, const uint8_t *sel,
                       const uint64_t *off, uint64_t *hist, int64_t hist_cap, const int32_t *level, int levels, void *stream);
int tomo_cc_level_sums(const int64_t *table, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint64_t *off,
                       const uint32_t *slot, const uint64_t *hist, int64_t hist_cap, const double *w, int nz, int levels,
                       int64_t *voxels, double *volume, int64_t *labels, int64_t cap_sel, void *stream);
/* Caliper (Feret) diameters and the oriented box per component (no counterpart in the reference): the extent of a component
 * between two parallel planes with unit normal u = (u_z, u_y, u_x), float64; u and -u give the same width.
 * Coordinates: those of the distance transform.  Voxel (k, j, i) sits at (zc[k], yt[j], xt[i]) = (zc[k], j * mm_y, i * mm_x),
 * the inner entries of the tables of tomo_edt_distance; d_k is the depth of slice k.
 * Shared directions: M directions for all components, as three host-built float64 tables PZ[m][k] = zc[k] * u_z, PY[m][j] =
 * yt[j] * u_y, PX[m][i] = xt[i] * u_x.  The projection of a voxel is p = ((PZ[m][k] + PY[m][j]) + PX[m][i]) + 0.0: additions
 * only, in this order; the + 0.0 turns -0.0 into +0.0 so that a maximum of keys is well defined.
 * Extent: centres (H == NULL): hi = max p, lo = min p over the voxels of the component.  voxels: the union of the voxel boxes,
 * hi = max (p + H[m][k]), lo = min (p - H[m][k]), H[m][k] = 0.5 * ((|u_z| * d_k + |u_y| * mm_y) + |u_x| * mm_x) built on the host:
 * a single voxel reads its own box width along u, not 0.  width = hi - lo in both cases.
 * Per-component directions: the three directions of component c are the rows a = (a_z, a_y, a_x) of axes[slot[c]] (the
 * principal axes of tomo_cc_moments).  No table per component, so the kernel multiplies: p = ((zc[k] * a_z + yt[j] * a_y) +
 * xt[i] * a_x) + 0.0 and H = 0.5 * ((|a_z| * d_k + |a_y| * mm_y) + |a_x| * mm_x), every product and sum rounded on its own,
 * never contracted.
 * Every operation is monotone in i, so hi / lo of a run [s, e) are attained at s or e - 1: the kernels evaluate the two ends of
 * every run only.  One thread per row (the row pass); results go to the compacted row slot[c] of the SELECTED components
 * (tomo_cc_select: sel, slot, tot[5]) as order-preserving uint64 keys of the float64 by 64-bit atomicMax / atomicMin -- integer
 * atomics only: the same bytes on every run.
 *   tomo_cc_caliper       hi, lo uint64[cap_sel][M], initialised here: the keys of hi / lo of selected component c + 1 in row
 *                         slot[c]; pz float64[M][nz], py [M][ny], px [M][nx], ph = H float64[M][nz] or NULL (centres)
 *   tomo_cc_caliper_axes  the same with M = 3 and the component's own directions: axes float64[cap_sel][9], zc float64[nz], yt
 *                         [ny], xt [nx], depth float64[nz] or NULL (centres; mm_y and mm_x are not read then)
 *   tomo_cc_caliper_rows  one thread per selected component: decodes hi / lo IN PLACE to float64[cap_sel][M], width
 *                         float64[cap_sel][M] = hi - lo, rows int64[cap_sel][4] row slot[c] = (c + 1, voxels, index of the largest
 *                         width, index of the smallest width; the lowest index among equals), ext float64[cap_sel][2] = (largest
 *                         width, smallest width)
 * tot[5] > cap_sel or tot[1] > cap: bit 1 of tot[2], nothing is written; a run id outside the tables, a slot outside cap_sel or
 * a selected component no voxel reached: bit 2.  TOMO_E_ARG for a null pointer (ph / depth excepted), hi == lo, a non-positive
 * size or M, and with depth a pixel size that is not positive and finite; TOMO_E_SIZE from 2^31 words, runs, components or
 * selected components, 524 280 directions or 2^57 cells on. */
int tomo_cc_caliper(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                    const uint32_t *rank, unsigned long long *tot, const uint8_t *sel, const uint32_t *slot, int64_t cap,
                    const double *pz, const double *py, const double *px, const double *ph, int M, uint64_t *hi, uint64_t *lo,
                    int64_t cap_sel, void *stream);
int tomo_cc_caliper_axes(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs,
                         const uint32_t *parent, const uint32_t *rank, unsigned long long *tot, const uint8_t *sel,
                         const uint32_t *slot, int64_t cap, const double *axes, const double *zc, const double *yt, const double *xt,
                         const double *depth, double mm_y, double mm_x, uint64_t *hi, uint64_t *lo, int64_t cap_sel, void *stream);
int tomo_cc_caliper_rows(const int64_t *table, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint32_t *slot,
                         uint64_t *hi, uint64_t *lo, int M, double *width, int64_t *rows, double *ext, int64_t cap_sel, void *stream);
/* Geodesic distance inside the set voxels (no counterpart in the reference): the length in mm of the shortest path that never
 * leaves the object, from a set of seeds.
 * The metric, one definition.  Voxel (k, j, i) sits at (zc[k], j * mm_y, i * mm_x), the coordinates of tomo_edt_distance.  A step
 * goes from a set voxel to a set voxel that is its neighbour under the connectivity, 6 or 26: the 26-adjacency of the two ends
 * alone, no corner-cutting test -- the adjacency of tomo_cc_label_runs, so a path never leaves a component.  The weight of a step
 * is its Euclidean length, computed on the host in float64 as sqrt(((dx * mm_x)^2 + (dy * mm_y)^2) + dzc^2), dzc = zc[k + 1] -
 * zc[k] between slices k and k + 1, and rounded ONCE to float32: wxy float32[3] for the steps x, y, xy; wz float32[max(nz - 1,
 * 1)][4] for the steps z, zx, zy, zyx across the boundary between slice k and k + 1 (connectivity 6 reads x, y and z only).
 * dist(p) = the minimum over the paths from a seed to p of the left-to-right float32 sum of the weights: 0.0 at a seed that is
 * set, +inf at a set voxel no seed reaches and at every unset voxel; a seed on an unset voxel is ignored.  This is the path
 * length on the 6 / 26 lattice: exact along the lattice directions, an overestimate between them like any chamfer metric, and
 * a float32 sum carries float32's relative precision along a very long path.
 * The fixed point.  The device only adds and takes minima (no contraction): d' = fl32(d + w) is monotone in d, so the system
 * dist(p) = min(seed(p), min over neighbours q of fl32(dist(q) + w)) has a unique least fixed point below the seeded map, and
 * values only fall through a finite set.  Every order of relaxations, every tiling and every race between tiles ends at the same
 * bytes: those Dijkstra's algorithm with the same float32 additions returns.
 * Tiles: 8 x 8 x 64 voxels (z, y, x), one word of the bit volume wide; tile (bz, by, bx) has the number (bz * ty + by) * wx + bx,
 * ty = ceil(ny / 8).  dirty arrays: uint32 per tile, zero or one.
 *   tomo_geo_tiles       the number of tiles (< 0: error)
 *   tomo_geo_seed_bits   one pass over the volume: dist = 0.0 where bits & seeds, +inf elsewhere; dirty[t] = 1 for every tile that
 *                        holds a seed, and for every neighbouring tile next to a seed on a face, an edge or a corner of its tile
 *                        (a seed is a change no sweep made, so no sweep would announce it); the caller zeroes both dirty arrays
 *   tomo_geo_seed_index  dist is prefilled with +inf by the caller.  One thread per entry c < n writes 0.0 at the flat index
 *                        index[c] = (z * ny + y) * nx + x where sel is NULL or sel[c] is set, and marks the tiles likewise; an entry of all
 *                        ones is skipped; an index outside the volume or on an unset voxel sets bit 2 of counters[1] and writes
 *                        nothing
 *   tomo_geo_sweep       one relaxation sweep: one workgroup of 256 threads per tile.  A workgroup whose flag in dirty_cur is
 *                        clear returns at once, otherwise it clears that flag (only it reads it), loads its interior and a
 *                        one-voxel halo of dist into LDS (unset voxels and everything outside the stack: +inf) and relaxes the
 *                        interior to convergence against the fixed halo, in race-free rounds bounded by the number of interior
 *                        voxels; a tile that hits the bound marks itself in dirty_next.  If something changed it stores the
 *                        changed voxels, adds 1 to counters[0] (once per workgroup) and sets dirty_next of every neighbouring
 *                        tile (up to 26; 6: up to 6) next to a face, edge or corner voxel that changed.  Only the owning
 *                        workgroup writes a dist entry: no atomics on dist.  A neighbouring tile may read an interior while it
 *                        is written: a stale value is a valid upper bound, aligned 32-bit accesses do not tear, and the writer
 *                        marks the reader for the next sweep -- that is the whole correctness argument.  Nothing waits on
 *                        another workgroup.  The caller swaps the two dirty arrays between sweeps and stops at a sweep (a batch
 *                        of sweeps) that left counters[0] unchanged: all flags are clear then.
 *   tomo_geo_reach       out = the set voxels with dist <= max_mm as a bit volume; max_mm = +inf: with a finite dist
 * counters: unsigned long long[2], zeroed by the caller.  TOMO_E_ARG for a null pointer (sel excepted), a non-positive size or n,
 * dirty_cur == dirty_next, a connectivity other than 6 / 26, a max_mm that is negative or NaN; TOMO_E_SIZE from 2^31 tiles or
 * words on. */
int64_t tomo_geo_tiles(int nz, int ny, int nx);
int tomo_geo_seed_bits(const uint64_t *bits, const uint64_t *seeds, int nz, int ny, int nx, float *dist, uint32_t *dirty, void *stream);
int tomo_geo_seed_index(const uint64_t *bits, int nz, int ny, int nx, const uint64_t *index, const uint8_t *sel, int64_t n,
                        float *dist, uint32_t *dirty, unsigned long long *counters, void *stream);
int tomo_geo_sweep(const uint64_t *bits, int nz, int ny, int nx, int connectivity, const float *wxy, const float *wz, float *dist,
                   uint32_t *dirty_cur, uint32_t *dirty_next, unsigned long long *counters, void *stream);
int tomo_geo_reach(const uint64_t *bits, const float *dist, int nz, int ny, int nx, double max_mm, uint64_t *out, void *stream);
/* Geodesic zones of markers and the cut between them (csrc/geodesic.hip; no counterpart in the reference): which marker reaches
 * a voxel first through the object, and the voxels to clear so that touching objects come apart.  Coordinates, connectivity,
 * weights, tiles, dirty arrays and dist are those of the block above; its kernels are not touched.
 * Markers: int32 (nz, ny, nx).  A positive entry on a set voxel is a marker voxel with that label; entries <= 0 and entries on
 * unset voxels are ignored; labels need not be consecutive.
 * Zones, one definition.  dist = the geodesic distance from the marker voxels.  An edge q -> p between neighbouring set voxels is
 * TIGHT when fl32(dist(q) + w(q, p)) == dist(p) with dist(p) finite -- the float32 addition the distance sweep makes.  zone(p) =
 * the smallest marker label among the markers from which p can be reached along tight edges; 0 at unset voxels and at set voxels
 * no marker reaches.  A marker voxel keeps its label: no edge into a voxel at distance 0 is tight, the weights are positive.
 * This is the least fixed point of zone(p) = min(zone(p), zone(q) over tight q -> p) over a FIXED graph: unique, so every order,
 * tiling and race ends at the same bytes, also where dist stalled along a very long path (fl32(d + w) == d).  Distance and label
 * are NOT relaxed as a pair: fl32(d + w) maps different d to one sum, so the pair operator is not monotone and its result would
 * depend on the schedule.  Two phases: tomo_geo_sweep to its fixed point, then tomo_zone_sweep over the final dist.
 * The map holds 0 for "no zone" at every moment; the kernels order labels by (uint32)(zone - 1), under which 0 is the largest.
 *   tomo_zone_seed_labels  one pass over the volume: dist = 0.0 and zone = the label where the voxel is set and its marker entry is
 *                          positive, dist = +inf and zone = 0 elsewhere; dirty is marked as tomo_geo_seed_bits marks it
 *   tomo_zone_sweep        one label sweep, shaped like tomo_geo_sweep: one workgroup of 256 per tile, gone at once when its flag in
 *                          dirty_cur is clear.  It loads the tile and a one-voxel halo of dist (read only here) and of zone into
 *                          LDS, finds the tight edges into its interior voxels once, and lowers the interior labels against the
 *                          fixed halo in race-free rounds bounded by the number of interior voxels (a tile that hits the bound
 *                          marks itself in dirty_next).  It stores the labels that changed, adds 1 to counters[0] (once per
 *                          workgroup that changed something) and sets dirty_next of the neighbouring tiles next to a changed
 *                          face, edge or corner voxel (6: face neighbours only).  No atomics on the maps, nothing waits on
 *                          another workgroup.  To start the phase the caller sets EVERY flag of dirty_cur once (one fill; the
 *                          distance phase left both arrays clear): a tile without work changes nothing and marks nobody, so it
 *                          is out after the first sweep.  The caller swaps the arrays between sweeps and stops at a batch that
 *                          left counters[0] unchanged, as for tomo_geo_sweep.
 *   tomo_zone_cut          out = bits without the set voxels p that have a SET neighbour q under the connectivity with
 *                          0 < zone(q) < zone(p): the lower label keeps the contact, and afterwards no two voxels of different
 *                          zones are adjacent; a component without a marker is untouched.  A wave takes a word at a time, a lane
 *                          one bit, tail bits zero; it walks 32 consecutive words and then adds their cleared voxels to *counter
 *                          (zeroed by the caller) with one integer atomic per wave.  Any int32 map is
 *                          taken: entries <= 0 are no zone, entries on unset voxels are not read as neighbours.
 * TOMO_E_ARG for a null pointer, a non-positive size, a connectivity other than 6 / 26, dirty_cur == dirty_next, markers == zone,
 * dist == zone, out == bits or out == zone; TOMO_E_SIZE from 2^31 tiles or words on. */
int tomo_zone_seed_labels(const uint64_t *bits, const int32_t *markers, int nz, int ny, int nx, float *dist, int32_t *zone,
                          uint32_t *dirty, void *stream);
int tomo_zone_sweep(const uint64_t *bits, int nz, int ny, int nx, int connectivity, const float *wxy, const float *wz,
                    const float *dist, int32_t *zone, uint32_t *dirty_cur, uint32_t *dirty_next, unsigned long long *counters,
                    void *stream);
int tomo_zone_cut(const uint64_t *bits, const int32_t *zone, int nz, int ny, int nx, int connectivity, uint64_t *out,
                  unsigned long long *counter, void *stream);
/* Greyscale morphological reconstruction by dilation inside the set voxels (csrc/reconstruct.hip; no counterpart in the
 * reference): a map that rises under a ceiling, the primitive behind h-maxima, regional and extended maxima.  Tiles, dirty
 * arrays and the adjacency (6 or 26 between two SET voxels) are those of tomo_geo_sweep.
 * mask: float32 (nz, ny, nx), the ceiling f.  marker: float32 of the same shape.  Unset voxels and everything outside the stack
 * take no part: they are never read as neighbours, their mask and marker entries are not read at all, and g holds 0.0 there.
 * Order.  Values are ordered as float32 orders them, -0.0 is read as +0.0 (and written as +0.0), NaN on a set voxel is an
 * error.  The kernels compare an order-preserving uint32 key of the bit pattern -- 0x80000000 + magnitude for a positive
 * value, 0x80000000 - magnitude for a negative one -- never the floats, so no float mode or denormal setting matters.  The
 * keys of -inf .. +inf are consecutive integers: "the float just below v" is the value of key(v) - 1 (below +0.0 lies the
 * smallest negative denormal); nothing lies below -inf.
 * Reconstruction, one definition.  m' = min(marker, f).  g is the least fixed point above m' of
 *     g(p) = max(m'(p), min(f(p), max over the set neighbours q of g(q))).
 * The operator only takes minima and maxima of values already present: it is monotone, and values only rise, through the
 * finite set of the inputs.  Every order of updates, every tiling and every race between tiles therefore ends at the same
 * bytes.  It is the argument of tomo_geo_sweep turned round: a neighbouring tile may read an interior while it is written and
 * gets the old or the new value (aligned 32-bit accesses do not tear); a stale value is a valid LOWER bound of the fixed
 * point, and the writer marks the reader for the next sweep.
 * h-maxima: HMAX_h(f) = the reconstruction of fl32(f - h) under f, one float32 subtraction per voxel, h > 0 finite.  Regional
 * maxima: RMAX(f) = the set voxels with reconstruction(f, the float just below f) < f -- the plateau definition: a connected
 * set of equal values with no higher set neighbour (a plateau at -inf is not reported).  Extended maxima: RMAX(HMAX_h(f)).
 *   tomo_recon_seed   one pass over the volume: g = min(marker, f) on a set voxel, 0.0 on an unset one.  mode 0 reads `marker`;
 *                     mode 1 takes fl32(f - h) and mode 2 the float just below f (marker may be NULL in both; h is read in
 *                     mode 1 only).  counters[1] |= 8 when the mask or the marker of a set voxel is NaN (the caller raises
 *                     and discards g), |= 16 when some set voxel starts below its ceiling -- without that bit g is final
 *                     and no sweep is needed.  One atomic per wave at most, and none once the bits are up.
 *   tomo_recon_sweep  one sweep, shaped like tomo_zone_sweep: one workgroup of 256 per tile, gone at once when its flag in
 *                     dirty_cur is clear; otherwise it clears the flag.  A thread holds the ceiling and g of its 16 voxels in
 *                     registers (only the owner reads a ceiling); a tile whose voxels all sit at their ceiling returns there.
 *                     g with a one-voxel halo goes into LDS as keys (unset voxels and outside: key 0, below every value), and
 *                     the interior is raised against the fixed halo in race-free rounds bounded by the number of interior
 *                     voxels (a tile that hits the bound marks itself in dirty_next).  It stores the voxels that changed,
 *                     adds 1 to counters[0] (once per workgroup that changed something) and sets dirty_next of the
 *                     neighbouring tiles next to a changed face, edge or corner voxel (6: face neighbours only).  No atomics
 *                     on the maps, nothing waits on another workgroup.  To start, the caller sets EVERY flag of dirty_cur
 *                     once: a tile without work changes nothing and marks nobody.  The caller swaps the arrays between
 *                     sweeps and stops at a batch that left counters[0] unchanged, as for tomo_geo_sweep.
 *   tomo_recon_below  out = the set voxels with g < mask (by the keys) as a bit volume; a wave is one word, tail bits zero
 * counters: unsigned long long[2], zeroed by the caller.  TOMO_E_ARG for a null pointer (marker in modes 1 and 2 excepted), a
 * non-positive size, a mode other than 0 .. 2, an h that is not positive and finite in mode 1, a connectivity other than
 * 6 / 26, dirty_cur == dirty_next, g == mask, g == marker, g == bits, out == bits, out == mask or out == g; TOMO_E_SIZE from
 * 2^31 tiles or words on.  All of it is decided before any device use. */
int tomo_recon_seed(const uint64_t *bits, const float *mask, const float *marker, int mode, float h, int nz, int ny, int nx,
                    float *g, unsigned long long *counters, void *stream);
int tomo_recon_sweep(const uint64_t *bits, int nz, int ny, int nx, int connectivity, const float *mask, float *g,
                     uint32_t *dirty_cur, uint32_t *dirty_next, unsigned long long *counters, void *stream);
int tomo_recon_below(const uint64_t *bits, const float *mask, const float *g, int nz, int ny, int nx, uint64_t *out, void *stream);
/* Homotopic thinning of the bit volume: the curve skeleton (csrc/thin.hip; no counterpart in the reference).  One definition.
 * Topology.  Everything outside the stack is background.  The foreground X has connectivity n = 26 or 6, the background the
 * complementary one.  N(p) is the picture of the 26 neighbours of p, N18 its face and edge neighbours.
 *   T26(M)  the number of 26-connected components of M
 *   T6(M)   the number of 6-connected components of M n N18 that contain a 6-neighbour of p
 * p is SIMPLE under 26 when T26(X n N) == 1 and T6(~X n N) == 1, under 6 when T6(X n N) == 1 and T26(~X n N) == 1; an
 * isolated voxel is never simple.  p is an END when exactly one of its 26 neighbours is set.
 * Order.  One ITERATION is 48 sub-passes: the six directions in the order -z, +z, -y, +y, -x, +x (direction 0 .. 5), and
 * inside each direction the eight subfields s = 4 (z & 1) + 2 (y & 1) + (x & 1), ascending, on the stack's own indices.
 * Sub-pass (d, s) clears, all at once, every voxel p that is set, is no anchor, lies in subfield s, whose neighbour in
 * direction d is clear or outside the stack, that is simple and -- with curve -- is no end; every condition is evaluated on
 * the volume as it stood when the sub-pass began.  The result is the volume after the first iteration that cleared nothing.
 * Sound: two voxels of one subfield are never 26-neighbours, so "all at once" equals "one after the other in any order",
 * every single deletion is the deletion of a simple point, and components, cavities and handles are those of the input.
 * Deterministic, and in place: a candidate reads its own row, the rows y +- 1 and z +- 1 and the side bits of the neighbouring
 * words.  The rows y +- 1 and z +- 1 have another parity and are not written in this sub-pass; in its own row every bit it
 * reads lies at x +- 1, the other x-parity, which has the same value before and after any concurrent aligned 64-bit store of
 * that word.  No second buffer, nobody waits on anybody, the same bytes on every run and under every tiling.
 * curve = 0 gives the ultimate homotopic kernel (a ball becomes one voxel, a ring a closed one-voxel curve, a shell stays a
 * closed surface), curve = 1 the curve skeleton; curve with connectivity 6 is refused (the 26-neighbour end rule eats a
 * 6-connected staircase from its end).  The thinning is in voxel steps: spacing and slice depths play no part in it.
 *   tomo_thin_pass   one sub-pass (direction, subfield), in place.  anchors: a bit volume of voxels that are never cleared, or
 *                    NULL.  One workgroup of 256 per tile of tomo_geo_tiles (8 x 8 x 64); only the rows of the subfield's
 *                    (z & 1, y & 1) do anything, a wave is one word of such a row, a lane a bit: the candidates of a word come
 *                    from word-wide operations, the lane cuts its 27-bit picture out of wave-uniform words and COMPUTES the
 *                    two component counts as bit floods; the wave ballots and one lane stores word & ~ballot (tail bits zero).
 *                    No atomics on the volume, no table.  stamp: uint32 per tile, zeroed by the caller before the first
 *                    sub-pass of a thinning; tick: the 1-based number of the sub-pass within that thinning, ascending by one.
 *                    A tile is visited while stamp + 48 >= tick; a wave that clears something raises (atomicMax) the stamp of
 *                    its tile and of the neighbouring tiles next to a cleared face, edge or corner voxel to tick.  A voxel's
 *                    verdict in a kind of sub-pass can only change when its picture changed since that kind last ran, so
 *                    skipping changes the work and never the bytes.  The voxels cleared are added to counters[16 k], k = 0 .. 63
 *                    (one atomic per wave that cleared some, on one of 64 addresses 128 bytes apart: the waves of a
 *                    launch do not queue on one address); their sum is the count.
 *   tomo_thin_nodes  ends_out = the set voxels with exactly one set 26-neighbour, junctions_out = those with three or more, as
 *                    bit volumes (every word written, tail bits zero).  counters[0 .. 3] += voxels, ends, junctions, isolated
 *                    voxels (no set neighbour).
 *   tomo_thin_count  over the run tables of a labelled volume (tomo_cc_label_runs; arguments and guards as tomo_cc_value_max,
 *                    selection as tomo_cc_value_rows): out[columns * slot[c] + column] += the set bits of `other`, a second
 *                    bit volume of the same shape, under the x-runs of the selected component c + 1.  One thread per word: the
 *                    popcount of other & run mask, one 64-bit atomicAdd per run with a count.  out: int64 (cap_sel, columns),
 *                    zeroed by the caller.
 * counters: unsigned long long[1024] / [4], zeroed by the caller.  TOMO_E_ARG for a null pointer (anchors excepted), a
 * non-positive size, a connectivity other than 6 / 26, a direction outside 0 .. 5, a subfield outside 0 .. 7, curve with
 * connectivity 6, anchors == bits, a tick of 0 or within 48 of 2^32, an output that is an input, a column outside
 * 0 .. columns - 1; TOMO_E_SIZE from 2^31 words, tiles, runs, components or selected components on.  All of it is decided
 * before any device use. */
int tomo_thin_pass(uint64_t *bits, const uint64_t *anchors, int nz, int ny, int nx, int connectivity, int curve, int direction,
                   int subfield, uint32_t *stamp, uint32_t tick, unsigned long long *counters, void *stream);
int tomo_thin_nodes(const uint64_t *bits, int nz, int ny, int nx, uint64_t *ends_out, uint64_t *junctions_out,
                    unsigned long long *counters, void *stream);
int tomo_thin_count(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                    const uint32_t *rank, unsigned long long *tot, const uint64_t *other, const uint8_t *sel, const uint32_t *slot,
                    int64_t *out, int column, int columns, int64_t cap, int64_t cap_sel, void *stream);
/* The branch table of a skeleton (csrc/branches.hip; no counterpart in the reference; AnalyzeSkeleton in BoneJ / MorphoLibJ and
 * skan answer the same question).  One definition.
 * S is any bit volume -- usually a skeleton, nothing assumes thinness.  Adjacency is always 26, outside the stack nothing is
 * set, deg(p) is the number of set 26-neighbours of a set voxel p.
 *   R  the REGULAR voxels: deg == 2.        N = S \ R  the NODE voxels: ends (deg 1), isolated voxels (0), junction voxels (>= 3).
 *   A BRANCH is a 26-connected component of R.  Inside R a voxel has at most two R-neighbours: a path or a closed cycle.
 *   A NODE is a 26-connected component of N.  An end voxel next to a junction voxel belongs to that junction's node (a
 *   one-step spur is part of its node, no branch); a two-voxel object is one node without a branch.  A node is a FREE END when
 *   it has exactly one voxel and that voxel has deg 1.
 * An EDGE is an unordered pair of 26-adjacent set voxels: R-R inside one branch, N-N inside one node, R-N an ATTACHMENT of a
 * branch to a node.  A path has exactly two attachments, counted with multiplicity (both may go to one node, or to one voxel),
 * a cycle none.
 * Length.  An edge belongs to a branch when at least one of its ends does.  It is counted once, at a regular voxel p of the
 * branch: for a neighbour q in N always, for a neighbour q in R only when q is raster-later (one of the 13 forward neighbours
 * of tomo_contact_count).  The count is filed in the slice k of p and in the column of tomo_cc_surface_hist for q - p: 0, 1, 2 =
 * x, y, xy in the slice, 3 .. 6 = z, xz, yz, xyz towards slice k + 1, 7 .. 10 the same towards k - 1; so the entries of a branch
 * stay inside the index box of its own voxels.  length = the sequential float64 sum of (double)count[k][c] * steps[k][c] in
 * ascending k, then ascending c, no product contracted into an FMA -- tomo_cc_surface with directions == 13 and F = steps, the
 * (nz, 11) table of step lengths sqrt(((dx mm_x)^2 + (dy mm_y)^2) + dzc^2), dzc = zc[k + 1] - zc[k] upward, zc[k] - zc[k - 1]
 * downward, 0.0 where that slice does not exist.  The length includes the two attaching steps.
 * Rows are in ascending label of the labelling of R under 26 (tomo_cc_label_runs), node rows in that of N.
 *   tomo_branch_split   regular_out = R, nodes_out = N as bit volumes (every word written, tail bits zero); counters[0 .. 3] +=
 *                       voxels, regular voxels, node voxels, isolated voxels.  tomo_thin_nodes' pass: a wave is a word, a lane
 *                       a bit; no atomics on the volumes.
 *   tomo_branch_hist    the histogram of the steps: arguments as tomo_cc_surface_hist over the run tables of R, then other = the
 *                       bits of S.  hist uint64[11 * hist_cap], zeroed here: hist[11 * (off[c] + z - zmin[c]) + 0 .. 10] by the
 *                       counting rule above, for the selected branches.  One thread per row of R: the rows in front of a voxel
 *                       are read from S alone, the rows behind it from S and R (14 row windows), popcounts under the run
 *                       masks, integer atomics only.  Guards: the bits of tomo_cc_surface_hist in tot[2].
 *   tomo_branch_attach  over the same tables and the selection of tomo_cc_select: attach uint64 (cap_sel, 2) and attach_count
 *                       uint64 (cap_sel), initialised here to (all ones, 0) and 0; per selected branch the minimum / maximum
 *                       (64-bit atomicMin / atomicMax) of the flat index (z * ny + y) * nx + x of every node voxel beside one of
 *                       its voxels, and the attachments added up.  A wave sends an atomic only for a run with an attachment.
 *   tomo_branch_lookup  labels_out[i] = the label (1-based) under the given run tables of the voxel at flat index queries[i];
 *                       0 where the voxel is clear and where the query is negative or past the volume.  One thread per query.
 *                       The tables hold no run starts: the run of a voxel is counted from the start bits of its row
 *                       (as tomo_cc_expand does), not searched.
 *   tomo_branch_clear   out (!= in, != bits) = in & ~(the runs of `bits` whose component c has flagged[c] != 0); flagged uint8
 *                       [n_flagged], n_flagged = the components of the tables.  One thread per word, as tomo_cc_fill_map; tail
 *                       bits of out are zero.  Pruning applies it twice: the tables of R with the flags of the branches, then
 *                       the tables of N with the flags of their free ends.
 * TOMO_E_ARG for a null pointer, a non-positive size, an output that is an input or another output; TOMO_E_SIZE from 2^31
 * words, runs, components, selected components or queries on.  All of it is decided before any device use.  Nobody waits on
 * anybody; the bytes are the same on every run. */
int tomo_branch_split(const uint64_t *bits, int nz, int ny, int nx, uint64_t *regular_out, uint64_t *nodes_out,
                      unsigned long long *counters, void *stream);
int tomo_branch_hist(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                     const uint32_t *rank, unsigned long long *tot, const int64_t *table, int64_t cap, const uint8_t *sel,
                     const uint64_t *off, uint64_t *hist, int64_t hist_cap, const uint64_t *other, void *stream);
int tomo_branch_attach(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                       const uint32_t *rank, unsigned long long *tot, const uint64_t *other, const uint8_t *sel, const uint32_t *slot,
                       uint64_t *attach, uint64_t *attach_count, int64_t cap, int64_t cap_sel, void *stream);
int tomo_branch_lookup(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                       const uint32_t *rank, unsigned long long *tot, int64_t cap, const int64_t *queries, int64_t n,
                       int64_t *labels_out, void *stream);
int tomo_branch_clear(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                      const uint32_t *rank, unsigned long long *tot, const uint8_t *flagged, int64_t n_flagged, const uint64_t *in,
                      uint64_t *out, void *stream);
/* A value along the components of a labelled volume: smallest, largest, where, and an exact mean (csrc/profile.hip; no
 * counterpart in the reference; Tb.Th along the skeleton in BoneJ, the throat radius of a pore-network model).  One definition.
 * values: float32 (nz, ny, nx).  A value is ADMITTED when its bit pattern is below 0x49800000: 0.0 <= v < 2^20, finite, not -0.0;
 * for those the unsigned order of the bit patterns is the float order.  Per component c + 1 of the run tables, over its voxels:
 *   lo, hi             the smallest and the largest bit pattern
 *   lo_first, hi_first the smallest flat index (z * ny + y) * nx + x whose value has the bits lo[c] / hi[c]
 *   sum                the int64 sum of q(v) = (int64) rint((double)v * 65536.0): fixed point at 2^-16.  The product is exact in
 *                      float64, rint rounds half to even, integer adds commute -- the same bytes on every run and under every
 *                      order; 2^27 voxels of the largest admitted value fit.  mean = ((double)sum / 65536.0) / voxels on the host.
 * The value of an unset voxel is never read.  A set voxel with a value that is not admitted raises bit 3 (8) of tot[2] and takes
 * no part.  On the run tables of the REGULAR voxels of a skeleton (tomo_branch_split) with the distance map of the object, the
 * rows are the radii along the branches; the nodes take tomo_cc_value_max / tomo_cc_value_first under their own tables.
 *   tomo_profile_stats  arguments and guards as tomo_cc_value_max.  lo uint32[cap] (set to all ones here), hi uint32[cap] and sum
 *                       int64[cap] (zeroed here).  One wave per word, one lane per bit; a word without a set bit leaves before
 *                       the map is touched.  Per run of a word one wave reduction each for min, max and the sum and at most three
 *                       atomics from one lane; a minimum or maximum is sent only where it beats what a plain load shows.
 *   tomo_profile_where  after it, on the same arrays: lo_first, hi_first uint64[cap], set to all ones here; per run at most two
 *                       64-bit atomicMin, again only below what a plain load shows.
 *   tomo_profile_rows   out int64[cap_sel][7] row slot[c] = (c + 1, voxels, lo[c], hi[c], sum[c], lo_first[c], hi_first[c]) for
 *                       the components tomo_cc_select selected; tot[5] > cap_sel: bit 1 of tot[2], nothing is written.
 * TOMO_E_ARG for a null pointer, a non-positive size, two of the arrays of a call being one, or one of them over the bits or the
 * map (tomo_profile_rows: over the table); TOMO_E_SIZE from 2^31 words, runs, components or selected components on.  All of it is
 * decided before any device use.  Integer atomics only, nobody waits on anybody. */
int tomo_profile_stats(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                       const uint32_t *rank, unsigned long long *tot, const float *values, uint32_t *lo, uint32_t *hi, int64_t *sum,
                       int64_t cap, void *stream);
int tomo_profile_where(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                       const uint32_t *rank, unsigned long long *tot, const float *values, const uint32_t *lo, const uint32_t *hi,
                       uint64_t *lo_first, uint64_t *hi_first, int64_t cap, void *stream);
int tomo_profile_rows(const int64_t *table, const uint32_t *lo, const uint32_t *hi, const int64_t *sum, const uint64_t *lo_first,
                      const uint64_t *hi_first, int64_t cap, unsigned long long *tot, const uint8_t *sel, const uint32_t *slot,
                      int64_t *out, int64_t cap_sel, void *stream);
/* Chord lengths of the volume as a whole (csrc/chords.hip; no counterpart in the reference): the chord-length distribution per
 * lattice direction, from which the host derives the lineal-path function, the mean intercept length (MIL) and the MIL fabric
 * tensor.  No labelling: a network, a foam or a packed bed may be one component.  One definition.
 * DIRECTIONS: the 13 forward steps s = (dz, dy, dx) in {-1, 0, 1}^3 with the first non-zero entry positive, in ascending tuple
 * order -- the table of tomo_cc_breadth_hist's families, read as steps:
 *     (0,0,1) (0,1,-1) (0,1,0) (0,1,1) (1,-1,-1) (1,-1,0) (1,-1,1) (1,0,-1) (1,0,0) (1,0,1) (1,1,-1) (1,1,0) (1,1,1)
 * CHORD: everything outside the stack is background (the distance transform's convention).  A chord of direction s is a maximal
 * sequence of set voxels p, p + s, .., p + (n - 1) s: its predecessor p - s and its successor p + n s are each either clear or
 * outside the stack; n >= 1 is its length in voxels.  Every set voxel lies in exactly one chord per direction.  A chord is a
 * BORDER chord when its predecessor or its successor is outside the stack.
 * STEP LENGTH: l_s(k) = sqrt(((dz d[k])^2 + (dy mm_y)^2) + (dx mm_x)^2) in float64, d[k] the depth of slice k: the path through
 * the voxel's own box (the convention of the caliper's extent = "voxels").  FIXED POINT: q_s(k) = rint(l_s(k) * 65536) as int64,
 * half to even, made on the host (tomo_profile_stats' rule): steps_q int64[nz][13].
 * TABLES: int64[13][lmax + 1], lmax >= max(nz, ny, nx), zeroed here; column 0 stays 0.  counts[m][n] = the chords of direction
 * m and length n; border[m][n] = those of them that are border chords; sum_q[m][n] = the sum of q_s(k) over the voxels (k their
 * slice) of the chords in that bin: with varying depths the length in mm of a chord with dz != 0 is no function of n, and
 * sum_q / counts / 65536 is the mean length in mm of the bin from integers alone.  For every m the sum over n of n * counts[m][n]
 * is the popcount of the volume.
 *   tomo_chord_hist  the directions led by z: one thread per position (j0, i0) of the slice plane, at step k at voxel
 *                    (k, (j0 + k dy) mod ny, (i0 + k dx) mod nx); where the index wraps the open chord ends as a border chord
 *                    and the next one starts as one.  Led by y: the same per slice, one thread per i0.  (0, 0, 1): the runs of the
 *                    rows.  Chords of fewer than 256 voxels are binned in LDS per workgroup and the non-zero bins added once;
 *                    a longer one goes to slot n mod 256 of a direct-mapped set of bins in LDS that the first length to come
 *                    claims, and straight to the tables only where another length holds its slot.  Integer atomics only: the
 *                    same bytes on every run.
 * TOMO_E_ARG for a null pointer, a non-positive size or lmax < max(nz, ny, nx); TOMO_E_SIZE from 2^31 words on. */
int tomo_chord_hist(const uint64_t *bits, int nz, int ny, int nx, const int64_t *steps_q, int64_t lmax, int64_t *counts,
                    int64_t *border, int64_t *sum_q, void *stream);
/* The two-point covariance of the volume as a whole (csrc/two_point.hip; no counterpart in the reference): S2(h), the chance
 * that two points a lag h apart both lie in the phase -- volume fraction, specific surface (the slope at the origin), correlation
 * length and its anisotropy, periodicity, the input of stochastic reconstruction.  No labelling.  One definition.
 * LAG: h = (hz, hy, hx), integers, over the box hz in [0, rz], hy in [-ry, ry], hx in [-rx, rx]; the half space suffices because
 * N(-h) = N(h).
 * COUNT: pairs[hz][hy + ry][hx + rx] = N(h) = #{p : p set, p + h set, both inside the stack}, int64 (rz + 1, 2 ry + 1, 2 rx + 1),
 * zeroed here.  No wrap-around and nothing outside the stack takes part: the non-periodic estimator.  N(0) is the popcount.  A
 * lag whose component reaches the size of its axis (hz >= nz, |hy| >= ny, |hx| >= nx) reads 0.  The plane hz = 0 holds both h and
 * -h and comes out point-symmetric; the kernel computes the whole box and mirrors nothing.
 * DENOMINATOR (host, closed form): P(h) = max(0, nz - hz) max(0, ny - |hy|) max(0, nx - |hx|), the pairs of voxels of the stack a
 * lag h apart; S2(h) = N(h) / P(h), NaN where P = 0; S2(0) is the volume fraction.
 * LIMITS: every r >= 0; rx <= 63 (a shifted word then comes from a word and one neighbour); rz <= nz - 1, ry <= ny - 1 and
 * rx <= nx - 1 are NOT required.  The callers keep words * lags within a work budget (pipeline.TWO_POINT_WORK_BUDGET = 2^42).
 * TAIL BITS of the input are never trusted (cc_word / cc_word_or0 of cc_runs.h).  Integer adds only: the same bytes on every run
 * and under every grid.  The table is a function of index lags alone: the spacing and the slice depths enter on the host.
 *   tomo_two_point  grid (planes (hz, hy) that can hold a pair, chunks of the word space), 256 threads: a thread takes word A of
 *                   row (k, j) and the words Bm, B0, Bp of the partner row (k + hz, j + hy), skipped outside the stack, and adds
 *                   popcount(A & shift(B, hx)) for every hx of a variant RX in {8, 16, 32, 63}, the smallest >= rx, to 2 RX + 1
 *                   32-bit accumulators in registers (the loop over hx unrolled when compiled: immediate shifts, static
 *                   indices); a wave whose A words are all zero skips the word.  At the end one wave sum per accumulator, the wave
 *                   sums combined in LDS, ONE 64-bit add per workgroup and lag of the box.  A chunk has at most 2^24 words, so a
 *                   workgroup's sum stays below 2^30 and no 32-bit sum can wrap.
 * TOMO_E_ARG for a null pointer, a non-positive size, a negative r or rx > 63; TOMO_E_SIZE from 2^31 words on or for a table of
 * 2^31 entries or more.  A refused call writes nothing. */
int tomo_two_point(const uint64_t *bits, int nz, int ny, int nx, int rz, int ry, int rx, int64_t *pairs, void *stream);
/* The contact table between zones (csrc/contacts.hip; no counterpart in the reference): which zones touch, over how large an
 * interface, how wide the throat between them is and how long the way across.  One definition.
 * zones: int32 (nz, ny, nx), tomo_zone_sweep's map or any map.  A voxel TAKES PART when it is set and its entry is positive.
 * A CONTACT PAIR is an unordered pair {p, q} of voxels that take part, are 26-neighbours and have zones(p) != zones(q).  It is
 * counted exactly once, at the raster-earlier voxel p, which looks at its 13 forward neighbours: (0, 0, +1) in its row,
 * (0, +1, -1 .. +1) in the next row of the slice, (+1, -1 .. +1, -1 .. +1) in the next slice.  Neighbours outside the stack do
 * not exist; a row never sees the end of the previous row.  The pair belongs to the ZONE PAIR (a, b) = (min, max) of the two
 * labels, to slice k = the slice of p (the lower of the two) and to one of the seven direction classes of tomo_cc_surface_hist,
 * in that order: x, y, xy, z, xz, yz, xyz.  Per zone pair:
 *   pairs        the contact pairs;  pair_counts[7] the same per class;  z_lo, z_hi the lowest and the highest k
 *   first_index  the smallest flat index (z * ny + y) * nx + x of a p
 *   area         the sequential float64 sum, in ascending k and within a slice in ascending class c, of
 *                (double)count[k][c] * F[k * 11 + c], F = the (nz, 11) table of tomo_cc_surface: columns 0 .. 2 use the slice's
 *                own depth, 3 .. 6 are the columns towards slice k + 1.  One adjacent pair of unlike voxels is one crossing of
 *                the interface by a lattice line, so the factor is that of the surface area.  directions == 3: x, y and z only.
 *   value_max    with `values` (float32 (nz, ny, nx), NaN-free; -0.0 counts as +0.0): the largest value over all p and q of the
 *                zone pair's contact pairs;  value_index the smallest flat index that attains it
 *   path         with `dist` (float32, non-negative or +inf) and the step weights wxy, wz of tomo_geo_sweep: the minimum over the
 *                contact pairs of fl32(fl32(dist(p) + w(p, q)) + dist(q)), p the raster-earlier voxel; +inf where none is finite
 * The table is open-addressed over 64-bit keys (a << 32) | b -- never 0, so a zeroed table is empty -- of `cap` slots, cap a
 * power of two; a 64-bit mixer, linear probing, a slot claimed by ONE compare-and-swap.  No thread waits for another and a probe
 * ends after cap steps.  Integer atomics only: the same bytes on every run.
 *   tomo_contact_count   *counter = the contact pairs N (zeroed here), one atomic per wave at most
 *   tomo_contact_insert  clears the slot arrays, then per slot: keys, pairs (sum), z_lo (min, read as uint32), z_hi (max),
 *                        first_index (min), value_max (max of an order-preserving uint32 key; with values), path (min of the bit
 *                        pattern; with dist).  A lane that finds no slot adds its pairs to counters[0] (zeroed by the caller)
 *                        and drops them: the caller must then discard the table (from then on no wave probes it any more,
 *                        so counters[0] says that pairs were lost, not how many a full run would have lost).
 *   tomo_contact_hist    lookup only.  row_of_slot: the row of an occupied slot, -1 elsewhere; offset[row]: the first slice entry
 *                        of the row, its segment z_hi - z_lo + 1 entries long.  Clears hist (entries x 7 uint64) and, with
 *                        values, value_index (rows uint64); adds to hist[(offset[row] + k - z_lo) * 7 + class] and takes the
 *                        minimum index whose value equals the slot's maximum.  A key the table does not hold, or an entry
 *                        outside [0, entries), is never written: its pairs are added to counters[1].
 *   tomo_contact_finish  one thread per row: out[row * 17 ..] = a, b, pairs, pair_counts[7], the bits of area, z_lo, z_hi,
 *                        first_index, the bits of value_max (float32), value_index, the bits of path (float32); a row whose
 *                        segment does not fit adds 1 to counters[1] and is zeroed.
 * values, dist (with wxy, wz, path), value_max and value_index may be NULL together as stated.  TOMO_E_ARG for a null or aliased
 * pointer, a non-positive size, a cap that is no power of two, rows > cap, directions other than 3 / 13; TOMO_E_SIZE from 2^31
 * words on and for cap > 2^30. */
int tomo_contact_count(const uint64_t *bits, const int32_t *zones, int nz, int ny, int nx, unsigned long long *counter, void *stream);
int tomo_contact_insert(const uint64_t *bits, const int32_t *zones, int nz, int ny, int nx, const float *values, const float *dist,
                        const float *wxy, const float *wz, int64_t cap, uint64_t *keys, uint64_t *pairs, int32_t *z_lo, int32_t *z_hi,
                        uint64_t *first_index, uint32_t *value_max, uint32_t *path, unsigned long long *counters, void *stream);
int tomo_contact_hist(const uint64_t *bits, const int32_t *zones, int nz, int ny, int nx, const float *values, int64_t cap,
                      const uint64_t *keys, const int32_t *row_of_slot, const int32_t *z_lo, const uint32_t *value_max,
                      const int64_t *offset, int64_t rows, uint64_t *hist, int64_t entries, uint64_t *value_index,
                      unsigned long long *counters, void *stream);
int tomo_contact_finish(int64_t rows, const int32_t *slot_of_row, int64_t cap, const uint64_t *keys, const uint64_t *pairs,
                        const int32_t *z_lo, const int32_t *z_hi, const uint64_t *first_index, const uint32_t *value_max,
                        const uint32_t *path, const uint64_t *value_index, const int64_t *offset, const uint64_t *hist, int64_t entries,
                        const double *F, int nz, int directions, int64_t *out, unsigned long long *counters, void *stream);
/* The same across Z-slabs (slab_components.py): rank r labels its slab with the functions above (n_r components); local
 * component c has the global id base_r + c, base_r = n_0 + .. + n_(r-1).  Pieces that touch across a cut are united, the roots
 * (smallest id = the piece with the component's first voxel) numbered in ascending id: scipy's numbering of the whole stack.
 * Run and component ids that arrive in a message are range-checked before they index anything (bit 2 of the flags).
 *   tomo_cc_slice_components  out int32[cap_out] = the local component (0-based) of every run of slice z, 0 behind them; bit 1 of
 *                             tot[2] if the slice has more than cap_out runs
 *   tomo_cc_seam_union        the seam below this slab: bits = the slab (its first slice is read), nb_bits = the lower
 *                             neighbour's last slice (ny rows), nb_row_off uint32[ny + 1] = tomo_cc_count_runs(nb_bits, 1, ny, nx),
 *                             nb_comp int32[nb_runs] = that slice's tomo_cc_slice_components.  win uint32[n_prev + n_own] = the
 *                             window of the id table, relative to base_(r-1): identity, then every pair of touching runs united.
 *                             seam_tot (device uint64[8]) is zeroed; [2] = flags
 *   tomo_cc_merge_tables      msg = the ranks' rows of `stride` int64: [0] flags, [1 .. 1 + n_r) the sizes of the rank's
 *                             components, from word off_win on its window as int32; bases = device int64[world + 1] (base_r,
 *                             the last = n_total); max_n / max_win = the largest n_r / window.  table uint32[n_total] = the root
 *                             of every id, num uint32[n_total] = at a root its 0-based number, sizes int64[n_total] of which the
 *                             first n = voxels of component 1..n; tot is zeroed, [0] = n_total, [1] = n, [2] = flags OR the
 *                             messages' flags.  blk: tomo_cc_scan_blocks(n_total) words
 *   tomo_cc_local_maps        per local component c of the slab at `base`: keep uint8[n_local] = the keep rule of tomo_cc_filter
 *                             on the global sizes (largest: the label goes to tot[3]) and / or label int32[n_local] = the global
 *                             label; either may be NULL, not both
 *   tomo_cc_filter_map        tomo_cc_filter with `keep` in place of the sizes      (tot: the slab's own counters)
 *   tomo_cc_fill_map          tomo_cc_filter_map ORed with a second volume: out (!= bits, != solid) = (solid ? solid : 0) | the bits
 *                             of the runs of `bits` whose component c has keep[c] != 0.  With the tables of a complement and
 *                             keep = the selection of its cavities (tomo_cc_select, enclosed), solid = the volume fills them,
 *                             solid = NULL extracts them.  One pass, one thread per word; tail bits of out are zero
 *   tomo_cc_expand_map        tomo_cc_expand with `label` in place of the numbering */
int tomo_cc_slice_components(int nz, int ny, int z, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                             const uint32_t *rank, unsigned long long *tot, int32_t *out, int64_t cap_out, void *stream);
int tomo_cc_seam_union(const uint64_t *bits, int ny, int nx, int connectivity, const uint32_t *row_off, int64_t cap_runs,
                       const uint32_t *parent, const uint32_t *rank, const unsigned long long *tot, const uint64_t *nb_bits,
                       const uint32_t *nb_row_off, const int32_t *nb_comp, int64_t nb_runs, int64_t n_prev, int64_t n_own,
                       uint32_t *win, unsigned long long *seam_tot, void *stream);
int tomo_cc_merge_tables(const int64_t *msg, int world, int64_t stride, int64_t off_win, const int64_t *bases, int64_t n_total,
                         int64_t max_n, int64_t max_win, uint32_t *table, uint32_t *num, int64_t *sizes, uint64_t *blk,
                         unsigned long long *tot, void *stream);
int tomo_cc_local_maps(const uint32_t *table, const uint32_t *num, const int64_t *sizes, unsigned long long *tot, int64_t n_total,
                       int64_t base, int64_t n_local, int64_t min_voxels, int largest, uint8_t *keep, int32_t *label, void *stream);
int tomo_cc_filter_map(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                       const uint32_t *rank, unsigned long long *tot, const uint8_t *keep, int64_t n_local, uint64_t *out,
                       void *stream);
int tomo_cc_fill_map(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                     const uint32_t *rank, unsigned long long *tot, const uint8_t *keep, int64_t n_local, const uint64_t *solid,
                     uint64_t *out, void *stream);
int tomo_cc_expand_map(const uint64_t *bits, int nz, int ny, int nx, const uint32_t *row_off, int64_t cap_runs, const uint32_t *parent,
                       const uint32_t *rank, unsigned long long *tot, const int32_t *label, int64_t n_local, int32_t *labels,
                       void *stream);
/* Exact Euclidean distance transform of the resident bits in millimetres (no counterpart in the reference;
 * scipy.ndimage.distance_transform_edt with a coordinate table per axis instead of one sampling per axis, so slice depths may
 * change from slice to slice).  zt / yt / xt: device float64[n + 2], strictly ascending: entry i + 1 = the centre of index i,
 * entries 0 and n + 1 = the VIRTUAL sites outside the volume.  inside != 0: the sites are the unset voxels and every virtual
 * position, the value at a set voxel is the distance to the nearest site and 0 at an unset one.  inside == 0: the sites are
 * the set voxels (virtual positions never are), the value at a set voxel is 0 and +inf everywhere if nothing is set.
 * d2 = ((dx^2 + dy^2) + dz^2) in float64, every d a difference of two table entries, no contraction; three separable passes
 * that each take the minimum over their line.  The volume is worked through in chunks of whole 64-column words of x:
 *   tomo_edt_workspace_bytes  bytes of the workspace for the widest chunk that fits budget_bytes (at least one word: the
 *                             result may exceed a smaller budget); linear in nz * ny * columns, never in the whole volume
 *   tomo_edt_chunk_columns    columns per chunk a workspace of that many bytes gives (TOMO_E_WORKSPACE below one word)
 *   tomo_edt_distance         out float32 (nz, ny, nx) = (float)sqrt(d2)
 *   tomo_edt_threshold        out uint64 (nz, ny, words) (!= bits): bit = d2 > r2 (keep_greater) or d2 <= r2, compared in
 *                             float64; tail bits zero; no float volume is made.  r2 >= 0
 *   tomo_edt_argmax           result device int64[2]: [0] = the bits of the largest float32 output value, [1] = the smallest
 *                             flat index (z * ny + y) * nx + x that attains it.  Per-thread partials folded by one workgroup
 *                             in a fixed order: no float atomics, the same on every run
 * The workspace is scratch: nothing is read from it that the call did not write.  bits is only read. */
int64_t tomo_edt_workspace_bytes(int nz, int ny, int nx, int64_t budget_bytes);
int64_t tomo_edt_chunk_columns(int nz, int ny, int nx, int64_t workspace_bytes);
int tomo_edt_distance(const uint64_t *bits, int nz, int ny, int nx, const double *zt, const double *yt, const double *xt, int inside,
                      float *out, void *workspace, int64_t workspace_bytes, void *stream);
int tomo_edt_threshold(const uint64_t *bits, int nz, int ny, int nx, const double *zt, const double *yt, const double *xt, int inside,
                       double r2, int keep_greater, uint64_t *out, void *workspace, int64_t workspace_bytes, void *stream);
int tomo_edt_argmax(const uint64_t *bits, int nz, int ny, int nx, const double *zt, const double *yt, const double *xt, int inside,
                    int64_t *result, void *workspace, int64_t workspace_bytes, void *stream);
/* Local thickness (Hildebrand & Ruegsegger) and ball openings by levels, on the coordinates and the background of the
 * transform above.  D2(q) = the float64 squared inside distance of set voxel q, |pq|^2 = ((dx^2 + dy^2) + dz^2) in float64,
 * every d a difference of two table entries, no contraction.  For ascending squared radii r_1^2 < ... < r_K^2
 *     level(p) = max{ k : there is a set voxel q with D2(q) >= r_k^2 and |pq|^2 < r_k^2 }      at a set voxel p,
 * 0 without such a k and at an unset voxel: {D2 >= r_k^2} are the centres where the OPEN ball of radius r_k fits, {level
 * reaches k} is the opening of the volume by that ball.  Digital openings are not monotone in r, hence the maximum.  One
 * outside transform of a bit volume per level:
 *   tomo_edt_squared           out float64 (nz, ny, nx) = d2 of tomo_edt_distance, unrounded (+inf without a site)
 *   tomo_edt_at_least          out uint64 (nz, ny, words) (!= bits): bit = set in bits && d2 >= r2, d2 float64 (nz, ny, nx) as
 *                              tomo_edt_squared wrote it; tail bits zero; no workspace.  r2 >= 0
 *   tomo_edt_cover             one level: the outside transform of `sites` (virtual positions never sites); where d2 < r2 at a
 *                              set voxel of `bits`, map int32 (nz, ny, nx) = level (>= 1); every other entry is left alone, so
 *                              levels run ascending over one zeroed map.  An unset voxel is never written, whatever d2 reads
 *   tomo_edt_threshold_masked  out uint64 (nz, ny, words) (!= sites, != mask) = mask & (d2 >= r2), or mask & (d2 < r2) with
 *                              keep_less, d2 the transform of `sites`; tail bits zero; no float volume is made.  The ball
 *                              opening is two calls: (bits, inside = 1, keep_less = 0, mask = bits) gives the eroded set,
 *                              (eroded, inside = 0, keep_less = 1, mask = bits) the opening
 *   tomo_edt_thickness_finish  map int32 -> float32 IN PLACE: values[level - 1] (device float32[levels], made on the host) at
 *                              a set voxel of level >= 1, +0.0 at every other voxel; counts int64 (nz, levels + 1) is zeroed
 *                              and then holds the set voxels of slice z at level l in [z][l] (column 0: set, below r_1).
 *                              Integer atomics only: the same bytes on every run.  levels >= 0
 * TOMO_E_ARG for a null pointer, a size < 1, r2 < 0 or NaN, level < 1 or an output that is one of the inputs, before any launch. */
int tomo_edt_squared(const uint64_t *bits, int nz, int ny, int nx, const double *zt, const double *yt, const double *xt, int inside,
                     double *out, void *workspace, int64_t workspace_bytes, void *stream);
int tomo_edt_at_least(const double *d2, const uint64_t *bits, int nz, int ny, int nx, double r2, uint64_t *out, void *stream);
int tomo_edt_cover(const uint64_t *sites, const uint64_t *bits, int nz, int ny, int nx, const double *zt, const double *yt,
                   const double *xt, double r2, int level, int32_t *map, void *workspace, int64_t workspace_bytes, void *stream);
int tomo_edt_threshold_masked(const uint64_t *sites, int nz, int ny, int nx, const double *zt, const double *yt, const double *xt,
                              int inside, double r2, int keep_less, const uint64_t *mask, uint64_t *out, void *workspace,
                              int64_t workspace_bytes, void *stream);
int tomo_edt_thickness_finish(int32_t *map, const uint64_t *bits, int nz, int ny, int nx, const float *values, int levels,
                              int64_t *counts, void *stream);
/* image_loader.py:108 (`img >= threshold`) fused with the packing: grey = uint8 (nz, ny, nx) on the device. */
int tomo_pack_threshold(const uint8_t *grey, uint64_t *bits, int nz, int ny, int nx, int threshold, void *stream);
/* obj_exporter.py:17-38, byte for byte ("v %.6f %.6f %.6f" per vertex, "f a+1 b+1 c+1" per face), HOST arrays:
 * vertices nv x 3 float32 (vertex_is_double = 0) or float64 (1), faces nf x 3 int64, 0-based.  Formats in parallel
 * on `nthreads` host threads.  Returns 0, TOMO_E_ARG, or -errno when the file cannot be written. */
int tomo_obj_write(const char *path, const void *vertices, int vertex_is_double, int64_t nv, const int64_t *faces,
                   int64_t nf, int nthreads);
/* The same file written by several processes (a Z-slab job; BASELINE configs[3] "seam-free OBJ export"): every rank
 * formats ITS run of the vertex list (kind 0: float32 rows, 1: float64 rows) or of the face list (kind 2: int64 rows
 * holding GLOBAL 0-based vertex indices) in host memory, learns the size, and -- once the sizes of all ranks are known
 * -- writes the bytes at its offset of the shared file, which must exist.  Same formatter as tomo_obj_write: the file
 * equals the one written from the gathered mesh.  A block lives until tomo_obj_block_free. */
int tomo_obj_block_format(int kind, const void *h_rows, int64_t n, int nthreads, void **h_block, int64_t *h_nbytes);
int tomo_obj_block_pwrite(const char *path, int64_t offset, const void *h_block);
void tomo_obj_block_free(void *h_block);

/* ---------------------------------------------------------------- scalar field ("SDF") */
/* bits -> extended bits (reflect of the padded array + zero pad ring), see tomo_ext_*. */
int tomo_extend_bits(const uint64_t *bits, uint64_t *ext, int nz, int ny, int nx, int pad, void *stream);
/* surface_extractor.py:43-53 + the float32 cast of skimage's wrapper: pad, astype(float64),
 * gaussian_filter(sigma=0.5) (three 5-tap float64 correlate1d passes, axis 0,1,2, mode reflect),
 * cast to float32.  gaussian = 0 writes the raw 0/1 field (manifold=False). */
int tomo_field_fill(const uint64_t *ext, float *field, int nz, int ny, int nx, int pad, int gaussian,
                    unsigned long long *signs, uint8_t *gcls, void *stream);   /* `field` must be 128-byte aligned */
/* The Gaussian field straight from the plain bit volume (no tomo_extend_bits): the block forms the extended words
 * while it stages its input.  Same outputs as tomo_field_fill(gaussian = 1) on tomo_extend_bits(bits). */
int tomo_field_fill_bits(const uint64_t *bits, float *field, int nz, int ny, int nx, int pad, unsigned long long *signs,
                         uint8_t *gcls, void *stream);
/* The same, minus what nothing downstream can read: the float field is an intermediate of surface_extractor.py:43-55 that
 * marching cubes reads only at the corners of active cells, so constant tiles whose input is uniform within 3 voxels stay
 * unwritten (their floats are undefined afterwards).  Sign records / classes as above (both required here).  span_ws:
 * 4-byte aligned device scratch of tomo_field_span_bytes(nz, ny, nx, pad) bytes. */
int64_t tomo_field_span_bytes(int nz, int ny, int nx, int pad);
int tomo_field_fill_bits_sparse(const uint64_t *bits, float *field, int nz, int ny, int nx, int pad, unsigned long long *signs,
                                uint8_t *gcls, uint8_t *span_ws, void *stream);
/* Sign records (input of marching-cubes pass 1): uint64 [Nz][S][NyP][4], S = tomo_mc_segments_per_row(Nx, xorg),
 * NyP = tomo_sign_rows(Ny) (Ny rounded up to 16 so that 16-row groups of records are 512-byte aligned);
 * bit L of word k of record (Z, s, Y) = [field(Z, Y, column 256 s - 224 + 4 L + k) > iso].  tomo_field_fill writes
 * them as a by-product (iso 0.5) when `signs` is not NULL and gaussian = 1 (no zeroing needed; bits of columns outside
 * the padded row are unspecified and ignored by tomo_mc_classify).  Records come in GROUPS of 16 rows; gcls
 * (uint8 [Nz][NyP / 16][S], always passed together with signs) holds the class of every group: 0 / 1 = all bits 0 / 1
 * and the 16 records are NOT stored (70 % of the groups of an ellipsoid volume), 2 = the records are stored.
 * tomo_field_signs derives records from any float field for slices [z_begin, z_end) (all groups of class 2). */
int64_t tomo_sign_rows(int Ny);
/* Size (uint64 words) of the buffer passed as `signs` to tomo_field_fill. */
int64_t tomo_sign_buffer_words(int Nz, int Ny, int Nx, int xorg);
int tomo_field_signs(const float *field, int Nz, int Ny, int Nx, int64_t pitch, int xorg, double iso, int z_begin,
                     int z_end, unsigned long long *signs, uint8_t *gcls, void *stream);

/* ---------------------------------------------------------------- marching cubes (Lewiner MC33) */
/* skimage.measure.marching_cubes(volume, level) (surface_extractor.py:55) as five device passes.
 * A SEGMENT = 256 consecutive float columns of a field row (voxel X is in segment (X + xorg + 224) / 256);
 * nseg = Nz * Ny * tomo_mc_segments_per_row(Nx, xorg).
 * A voxel is ACTIVE when its 8 cube corners (neighbours clamped at the volume border) are not all on one side
 * of `iso` (a corner equal to iso counts as below, like the reference).
 * vertex/voxel key = (row << 22) | (X << 2) | slot, row = Z*Ny + Y; slot 0/1/2 = x/y/z edge owned by the
 * voxel, 3 = cell-centre vertex (voxel keys have slot 0).
 *
 * 1. classify: from the sign records, seg_cnt[seg] = number of active voxels of EVERY segment (uint32[nseg],
 *    seg = (Z*Ny + Y)*S + s) and, for every NON-EMPTY segment, seg_act[4*seg + k] = 64-bit mask whose bit L says
 *    voxel 4L+k of the segment (X = 256 s - 224 + 4L + k - xorg) is active (seg_act: uint64[4*nseg]; records of
 *    empty segments stay unwritten and are never read).  No float is read. */
int tomo_mc_classify(const unsigned long long *signs, const uint8_t *gcls, int Nz, int Ny, int Nx, int xorg,
                     unsigned long long *seg_act, uint32_t *seg_cnt, void *stream);
/* Segment-level scan: seg_aoff uint32[nseg + 1] = exclusive scan of seg_cnt, totals (device uint64[4]) =
 * {active voxels, 0, 0, 0}.  workspace: tomo_mc_scan_workspace_bytes(nseg) bytes. */
int tomo_mc_scan_segments(const uint32_t *seg_cnt, int64_t nseg, uint32_t *seg_aoff, unsigned long long *totals,
                          void *workspace, int64_t workspace_bytes, void *stream);
/* Exclusive scan of packed counts (low 16 bits -> off_a, high 16 bits -> off_b; both uint32[n + 1]; with off_b = NULL
 * the counts are plain numbers and off_a their exclusive scan), totals (device uint64[4]) = {sum low, sum high, 0, 0}.
 * workspace: tomo_mc_scan_workspace_bytes(n) bytes. */
int64_t tomo_mc_scan_workspace_bytes(int64_t n);
int tomo_mc_scan(const uint32_t *counts, int64_t n, uint32_t *off_a, uint32_t *off_b,
                 unsigned long long *totals, void *workspace, int64_t workspace_bytes, void *stream);
/* 2. list: vox_key[na] = keys of the active voxels, ascending (cell scan order), from seg_act. */
int tomo_mc_list(int Nz, int Ny, int Nx, int xorg, const uint32_t *seg_aoff, const unsigned long long *seg_act,
                 unsigned long long *vox_key, void *stream);
/* 3. eval: one MC33 evaluation per active voxel: vox_counts[na] = ntri << 16 | nvert,
 * vox_flags[na] = bit0/1/2 edge vertices, bit3 centre vertex. */
int tomo_mc_eval(const float *field, int Nz, int Ny, int Nx, int64_t pitch, int xorg, double iso,
                 const unsigned long long *vox_key, int64_t na, uint32_t *vox_counts, uint8_t *vox_flags, void *stream);
/* Capped variants: the caller launches them BEFORE it has read the segment scan's total (one host round trip less per
 * pass).  `cap` entries of buffer; list: segments that would not fit are skipped; eval: entries at and beyond *na_dev
 * (device memory) get count 0, so tomo_mc_scan over all `cap` counts yields the same totals.  The caller checks
 * na <= cap afterwards and falls back to the exact calls otherwise. */
int tomo_mc_list_capped(int Nz, int Ny, int Nx, int xorg, const uint32_t *seg_aoff, const unsigned long long *seg_act,
                        unsigned long long *vox_key, int64_t cap, void *stream);
int tomo_mc_eval_capped(const float *field, int Nz, int Ny, int Nx, int64_t pitch, int xorg, double iso,
                        const unsigned long long *vox_key, int64_t cap, const unsigned long long *na_dev,
                        uint32_t *vox_counts, uint8_t *vox_flags, void *stream);
/* 4. emit: vertices (key + raw MC position, (z,y,x) float32 as skimage returns them; keys ascending) and
 * triangles as provisional vertex indices (int32), in the reference's order and with the per-triangle
 * reversal of skimage/measure/_marching_cubes_lewiner.py:338.  totals[3] counts corners whose vertex was
 * not found (must stay 0).  z_offset (0 on one GPU) is added to the slice index of every vertex position before
 * rounding: a Z-slab rank emits positions in global padded coordinates. */
int tomo_mc_emit(const float *field, int Nz, int Ny, int Nx, int64_t pitch, int xorg, double iso,
                 const unsigned long long *vox_key, int64_t na, const unsigned long long *seg_act,
                 const uint32_t *seg_aoff, const uint32_t *vox_voff, const uint32_t *vox_foff, const uint8_t *vox_flags,
                 int z_offset, unsigned long long *vkey, float *vpos, int32_t *faces, unsigned long long *totals,
                 void *stream);   /* seg_act / seg_aoff: from classify / scan_segments (vertex lookup by ballot rank) */

/* 5. (manifold=False only) skimage's first-touch vertex numbering, which the reference returns unchanged when it
 * skips np.unique (surface_extractor.py:67-68): mode 0 writes created[na] = vertices each cell creates in the
 * serial scan; after an exclusive scan (tomo_mc_scan) mode 1 writes ft_rank[provisional vertex] = its number. */
int tomo_mc_first_touch(const float *field, int Nz, int Ny, int Nx, int64_t pitch, int xorg, double iso,
                        const unsigned long long *vox_key, int64_t na, const unsigned long long *seg_act,
                        const uint32_t *seg_aoff, const uint32_t *vox_voff, const uint8_t *vox_flags, int mode,
                        uint32_t *created, const uint32_t *base, int32_t *ft_rank, unsigned long long *totals, void *stream);

/* ---------------------------------------------------------------- "mc3": marching cubes + finalisation + unique in one chain
 * The production path for manifold=True (surface_extractor.py:55-72): same inputs as above (sign records -> tomo_mc_classify
 * -> seg_cnt / seg_act), then
 *   tomo_mc3_list      block sums of seg_cnt, one single-workgroup scan, list of active voxels; tot[0] = list length
 *   tomo_mc3_eval      one float64 evaluation per active voxel: MC33 tiling reference, vertex flags, vertex coordinates
 *                      along the owned edges (float32), counts reduced per block of 256 entries
 *   tomo_mc3_scan      single workgroup: block prefixes, totals (tot[1] vertices, tot[2] triangles), per-slice tables and
 *                      the offsets of the sort's segments (slice_tab: tomo_mc3_slice_table_words(Nz, Ny) uint32)
 *   tomo_mc3_vertices  FINAL vertex rows (-1 shift, slice-depth map, y / x scale: surface_extractor.py:57-65, :82-113) as
 *                      16-byte records {z', y', x', id}, partitioned per slice into in-plane / between-plane buckets,
 *                      with their 32-bit sort keys; vertex id = 4 * (list position of the owner voxel) + slot
 *   tomo_mc3_sort_rank_top / _fused  sort inside the buckets + gather: uniq rows in np.unique's order, table[id] = index;
 *                      tot[4] counts the places where the rows do not ascend strictly (0 <=> the result is exact)
 *   tomo_mc3_faces     final int64 triangles (reference order and winding) through table; tot[5] degenerate triangles
 *                      (the caller drops them), tot[6] corners without vertex (must stay 0)
 * Every kernel takes the list length / totals from `tot` (device uint64[8]): the chain can be enqueued into buffers sized
 * from a hint (cap list entries, cap_v vertices, cap_f triangles) before any count is known to the host; what does not fit
 * is flagged in tot[3] (1 list, 2 vertices, 4 triangles) and nothing is written past a buffer.
 * Buffers: seg_blk uint32[ceil(nseg / 256)], seg_aoff uint32[nseg + 1], vox_key uint64[cap], vox_loc uint32[cap],
 * vox_til int32[cap], vox_flags uint8[cap], vox_used uint16[cap] (cube edges with a vertex), vox_f3 / vox_c3 float[3 cap], blk3 uint32[3 ceil(cap / 256)],
 * vrec float[4 cap_v], keys / idx uint32[cap_v], uniq float[3 cap_v], table int32[4 cap], faces int64[3 cap_f]. */
int tomo_mc3_list(int Nz, int Ny, int Nx, int xorg, const uint32_t *seg_cnt, const unsigned long long *seg_act,
                  uint32_t *seg_blk, uint32_t *seg_aoff, unsigned long long *vox_key, int64_t cap, unsigned long long *tot,
                  void *stream);
int tomo_mc3_eval(const float *field, int Nz, int Ny, int Nx, int64_t pitch, int xorg, double iso,
                  const unsigned long long *vox_key, int64_t cap, const unsigned long long *tot, int z_offset,
                  uint32_t *vox_loc, int32_t *vox_til, uint8_t *vox_flags, uint16_t *vox_used, float *vox_f3, float *vox_c3,
                  uint32_t *blk3, void *stream);
int64_t tomo_mc3_slice_table_words(int Nz, int Ny);
int64_t tomo_mc3_sort_segments(int Nz, int Ny);      /* sort segments: per slice its plane (cut into bands of 512 owner rows when Ny > 1280) + the between-plane bucket */
int tomo_mc3_scan(int Nz, int Ny, int Nx, int xorg, const uint32_t *seg_aoff, const uint32_t *vox_loc, int64_t cap,
                  uint32_t *blk3, uint32_t *slice_tab, unsigned long long *tot, int64_t cap_v, int64_t cap_f, void *stream);
int tomo_mc3_vertices(int Nz, int Ny, int Nx, int xorg, const unsigned long long *vox_key, int64_t cap,
                      const unsigned long long *tot, const uint32_t *vox_loc, const uint8_t *vox_flags, const float *vox_f3,
                      const float *vox_c3, const uint32_t *blk3, const uint32_t *slice_tab, int z_offset, int shift,
                      const double *cum, int64_t ncum, const double *adj, int64_t nadj, float mm_y, float mm_x, float *vrec,
                      uint32_t *keys, uint32_t *idx, void *stream);
int64_t tomo_mc3_sort_workspace_bytes(int64_t cap_v, int64_t nseg);    /* nseg = tomo_mc3_sort_segments(Nz, Ny) */
/* The unique stage through rocPRIM's segmented sort (workspace: tomo_mc3_sort_workspace_bytes), and tot[7] = number of rows
 * with z' == z_top (the plane a Z-slab rank shares with the rank above; NaN: none). */
int tomo_mc3_sort_rank_top(const float *vrec, uint32_t *keys, uint32_t *idx, int64_t cap_v, int Nz, int Ny, const uint32_t *slice_tab,
                           unsigned long long *tot, float *uniq, int32_t *table, void *workspace, int64_t workspace_bytes,
                           float z_top, void *stream);
/* ABI 6, the default since round 4: the same stage -- np.unique(axis=0)'s order inside the buckets, rows, table, the count of
 * places that do not ascend strictly (tot[4]), the rows on z' == z_top (tot[7]) -- in ONE hand-written kernel (a workgroup per
 * segment: wave bitonic + merge rounds in LDS, rows gathered in sorted order), no library primitive, no workspace; `idx` of
 * tomo_mc3_vertices may be NULL for it.  A segment longer than 4 096 entries (1 024 for the clamped run of a padded stack's
 * first slices) sets the value 8 (bit 3) in tot[3]: repeat the stage with tomo_mc3_sort_rank_top (after zeroing tot[3], tot[4], tot[7]). */
int tomo_mc3_sort_rank_fused(const float *vrec, const uint32_t *keys, int64_t cap_v, int Nz, int Ny, uint32_t *slice_tab,
                             unsigned long long *tot, float *uniq, int32_t *table, float z_top, void *stream);
int tomo_mc3_faces(int Nz, int Ny, int Nx, int xorg, const unsigned long long *vox_key, int64_t cap, unsigned long long *tot,
                   const unsigned long long *seg_act, const uint32_t *seg_aoff, const uint32_t *vox_loc, const int32_t *vox_til,
                   const uint16_t *vox_used, const uint32_t *blk3, const int32_t *table, int64_t *faces, int64_t cap_f,
                   void *stream);

/* ---------------------------------------------------------------- mesh finalisation */
/* surface_extractor.py:57-65 + :82-113 on (V,3) float32 rows in place: -1 shift (if shift),
 * variable slice depth map of z (cum/adj float64 tables as the reference builds them; nadj = 0
 * skips it), y *= mm_y, x *= mm_x (float32). */
int tomo_vertex_finalize(float *vpos, int64_t nv, int shift, const double *cum, int64_t ncum,
                         const double *adj, int64_t nadj, float mm_y, float mm_x, void *stream);
/* The vertex half of surface_extractor.py:115-126 (np.unique(axis=0, return_inverse)) for arbitrary rows, on the device:
 * lexicographic (z,y,x) sort of the vertex rows, dedupe -> uniq (U,3), rank[V] = final index of every provisional vertex;
 * totals[0] = U.  Workspace size from tomo_mesh_unique_workspace_bytes. */
int64_t tomo_mesh_unique_workspace_bytes(int64_t nv);
int tomo_mesh_unique(const float *vpos, int64_t nv, float *uniq, int32_t *rank, unsigned long long *totals,
                     void *workspace, int64_t workspace_bytes, void *stream);
/* out[i] = index of query row i in the sorted duplicate-free row list uniq (nu x 3), -1 (and *missing += 1, a device
 * counter the caller zeroes) if it is not there.  Used by the Z-slab job for the shared-plane vertices. */
int tomo_mesh_lookup(const float *uniq, int64_t nu, const float *query, int64_t nq, int32_t *out,
                     unsigned long long *missing, void *stream);
/* Z-slab numbering without host round trips (scale-out of the path; no counterpart in the single-process
 * reference): all counts come from `tot` of the rank's mc3 chain (tot[1] rows, tot[7] of them on the shared top plane).
 *   tomo_slab_top_rows        msg float32[(cap + 1) * 3]: row 0 = {n_top as uint32 bits, 0, 0}, then the top-plane rows, zero
 *                             padded
 *   tomo_slab_lookup_summary  ONE launch for the lookup of a received message and this rank's summary:
 *                             out[i] (int32[cap]) = index of row i of `msg` in this rank's uniq, -1 past the message's count
 *                             or when the row is not there;
 *                             summary int64[8] = kept rows | rows of `msg` not found | flags (1 the chain's counts cannot be
 *                             trusted: a buffer overflowed, 2 rows not strictly ascending, 4 n_top > cap_top, 8 caller_flags
 *                             != 0) | rows | top rows | rows announced from below | list length | triangles -- what the
 *                             ranks all-gather.  The workgroup that finishes last writes it.  scratch: uint64[2] (a ticket
 *                             and the misses), zeroed once by the caller, left zero by every call.  msg == NULL (the lowest
 *                             rank): the summary alone, out and cap unused.
 *   tomo_mc3_faces_slab       tomo_mc3_faces with GLOBAL indices: row r of this rank's list (what `table` names) leaves as r +
 *                             this rank's offset (the sum of the lower ranks' kept rows in `gathered`, int64[world][8]) while
 *                             r < kept rows, and as ids_next[r - kept] (the `out` of the upper rank's lookup) + the upper
 *                             rank's offset for the rows on the shared top plane */
int tomo_slab_top_rows(const float *uniq, const unsigned long long *tot, int64_t cap_v, int64_t cap, float *msg, void *stream);
int tomo_slab_lookup_summary(const float *uniq, const unsigned long long *tot, int64_t cap_v, const float *msg, int64_t cap,
                             int32_t *out, int64_t cap_top, int64_t caller_flags, unsigned long long *scratch, int64_t *summary,
                             void *stream);
int tomo_mc3_faces_slab(int Nz, int Ny, int Nx, int xorg, const unsigned long long *vox_key, int64_t cap, unsigned long long *tot,
                        const unsigned long long *seg_act, const uint32_t *seg_aoff, const uint32_t *vox_loc, const int32_t *vox_til,
                        const uint16_t *vox_used, const uint32_t *blk3, const int32_t *table, int64_t *faces, int64_t cap_f,
                        const int64_t *gathered, int rank, int world, const int32_t *ids_next, int64_t cap_top, int64_t cap_v,
                        void *stream);
/* surface_extractor.py:128-149: out[0] = sum over faces of dot(v0, cross(v1,v2))/6 (float64
 * accumulation of float32 terms), out[1] = sum of 0.5*|cross(v1-v0, v2-v0)|.  out is zeroed by the
 * caller; tree reduction => parity with the reference's sequential sums is to 1e-6 rel, not bitwise. */
int tomo_mesh_volume_area(const float *verts, const int64_t *faces, int64_t nf, double *out, void *stream);

/* ---- GLB export (glb_exporter.py of the reference; tomography_3d_reconstructor_amd/glb_exporter.py) -------------------
 * Orientation contract (trimesh's fix_normals(multibody=False) = fix_winding + fix_inversion, written out):
 *  1. two faces are neighbours when they share an undirected edge that has exactly two faces;
 *  2. in each connected component the lowest-index face keeps its winding; every other face is reversed exactly when its
 *     parity to that face is odd; a component whose constraints contradict each other is left as given;
 *  3. if the signed volume of the result is < 0, every face is reversed.  Reversing is (a,b,c) -> (c,b,a).
 *
 * Normals contract (NORMAL is optional and has no counterpart in the reference's file; area-weighted vertex normals).
 * Inputs: the float32 POSITION rows exactly as the file stores them (float64 vertices are rounded first) and the faces
 * AFTER the orientation contract, i.e. the index buffer the file stores.  Columns keep the order given, like POSITION.
 *  1. face vector, in float64 from the float32 positions, no fused multiply-add: u = p1 - p0, w = p2 - p0,
 *     g = (u.y w.z - u.z w.y, u.z w.x - u.x w.z, u.x w.y - u.y w.x).  Not normalised (the sum is area-weighted); a face
 *     with a repeated index gives g = 0 by itself;
 *  2. vertex sum s_v = sum of g_f over the corners that name v (a face that names v twice counts twice -- with g = 0), in
 *     float64, ADDED IN ASCENDING FACE INDEX starting from +0.0: the result is a function of the input alone, the same
 *     bytes on every run and every schedule;
 *  3. q = s.x s.x + s.y s.y + s.z s.z (left to right).  If q is finite and > 0: n = s / sqrt(q) component by component in
 *     float64, then rounded to float32.  Otherwise (a vertex no face names, faces that cancel, overflow) n = (0, 0, 1) and
 *     a counter goes up by one: glTF forbids a zero-length normal.
 *
 * Multi-rank (the Z-slab job's export; every rank holds its own vertex rows and its own faces, faces in rank order, and a
 * face of rank r names rows of rank r or a prefix of rank r + 1's rows -- the GHOST rows of rank r, all on the plane the two
 * ranks share).  A SEAM EDGE is an undirected edge both of whose endpoints are ghost rows of the lower rank: the only kind
 * of edge that can have faces on two ranks.  The lower rank sends one record per seam edge of its table (key in the upper
 * rank's row numbers, face count, direction bits of its first two faces); the upper rank looks each one up in its own table
 * and corrects the four edge counters so that, summed over the ranks, they are tomo_mesh_edges' counters of the gathered
 * mesh: an edge with c_lo faces below and c_hi above counts once, in the class of c_lo + c_hi, and a pair with one face on
 * either side is inconsistent exactly when both run the edge the same way (row order is the same in local and in global
 * numbers).  With zero inconsistent pairs no face flips by rules 1-2, and rule 3 reads a sum of per-rank volumes.
 * Normals: rule 2 adds in ascending GLOBAL face index, and every face of a lower rank precedes every face of an upper one.
 * So the lower rank adds its faces' vectors to +0.0 for each ghost row, in ascending order, and hands the RAW float64 sums
 * up; the owner starts from them instead of +0.0 and goes on with its own faces: ((0 + g1) + g2) + g3 ... is the same
 * sequence of additions as on one GPU, hence the same bytes. */
/* glb_exporter.py:52-91 on the device.  z = verts[i * stride] (float32, or float64 when is_f64).  rgba: uint8 (nv, 4),
 * 4-byte aligned; 200,200,200,255 by default, 255,0,0,255 where enable1 && start1 <= z <= end1, then 0,0,255,255 where
 * enable2 && start2 <= z <= end2 (blue wins).  Comparisons in float64: the caller passes bounds already rounded the way
 * its NumPy promotes them. */
int tomo_layer_colors(const void *verts, int is_f64, int64_t nv, int64_t stride, double start1, double end1, int enable1,
                      double start2, double end2, int enable2, uint8_t *rgba, void *stream);
/* Bytes of the edge table for nf faces (nf < 2^31): an open-addressing hash of undirected edges, keys (min << 32) | max,
 * sized to at least 2x the 3 nf insertions. */
int64_t tomo_mesh_edge_table_bytes(int64_t nf);
/* Builds the edge table of faces (int64, nf x 3) over nv vertices (nv < 2^32) and counts, into counters[6] (zeroed by the
 * call): [0] boundary edges (1 face), [1] manifold edges (2), [2] non-manifold edges (>= 3), [3] inconsistent pairs (a
 * manifold edge both faces run in the same direction), [4] faces with an index outside [0, nv) (they add no edges; the
 * mesh is invalid when this is not 0), [5] degenerate faces (a repeated index; they add no edges).  Per key the table
 * holds the face count and the first two (face << 1 | direction) entries. */
int tomo_mesh_edges(const int64_t *faces, int64_t nf, int64_t nv, void *table, int64_t table_bytes, unsigned long long *counters,
                    void *stream);
/* Multi-rank, the lower rank's half: every entry of a table built by tomo_mesh_edges (nf faces, LOCAL indices: own rows, then
 * ghost rows from first_ghost on) whose two endpoints are >= first_ghost becomes one record of two uint64 in msg:
 * [0] = (lo - first_ghost) << 32 | (hi - first_ghost), the key in the upper rank's local indices; [1] = bits << 32 | face
 * count, bit 0 / 1 of bits = the direction of the first / second stored face.  *count (zeroed by the call) ends as the
 * number of such entries whatever cap is; at most cap records are written (cap = 0, msg = NULL: count only).  The order
 * of the records depends on the schedule; what tomo_mesh_seam_merge makes of them does not. */
int tomo_mesh_seam_edges(const void *table, int64_t table_bytes, int64_t nf, int64_t first_ghost, unsigned long long *msg,
                         int64_t cap, unsigned long long *count, void *stream);
/* Multi-rank, the upper rank's half: looks n records up in this rank's table (read only) and writes corr[4] (int64, zeroed
 * by the call): signed corrections to boundary / manifold / non-manifold edges and inconsistent pairs such that the sum
 * over the ranks of (tomo_mesh_edges' counters + corr) equals the counters of the gathered mesh. */
int tomo_mesh_seam_merge(const void *table, int64_t table_bytes, int64_t nf, const unsigned long long *msg, int64_t n,
                         int64_t *corr, void *stream);
int64_t tomo_mesh_orient_workspace_bytes(int64_t nf);
/* Rules 1-2 of the contract over a table built by tomo_mesh_edges (only needed when counters[3] > 0: otherwise no face
 * flips).  Union-find with parity: parent and parity in one 64-bit word, the larger root hooked under the smaller with
 * atomicCAS (the root is the lowest-index face whatever the schedule), then a verification pass over every manifold edge
 * marks the conflicting components.  flip: uint8[nf] (1 = reverse the face); counts[2] (zeroed by the call): components,
 * conflicting components. */
int tomo_mesh_orient(const void *table, int64_t table_bytes, int64_t nf, void *workspace, int64_t workspace_bytes, uint8_t *flip,
                     unsigned long long *counts, void *stream);
/* *out += sum over faces of dot(v0, cross(v1, v2)) / 6 (the terms of tomo_mesh_volume_area), the term negated where flip[f]
 * (flip may be NULL).  out is zeroed by the caller.  Rule 3 of the contract reads the sign. */
int tomo_mesh_signed_volume(const float *verts, const int64_t *faces, int64_t nf, const uint8_t *flip, double *out, void *stream);
/* Oriented faces: face f reversed when flip[f] (NULL: none) XOR (volume != NULL && *volume < 0).  out: uint32 (the GLB
 * index buffer, 4-byte aligned) or, with out_i64, int64 (8-byte aligned). */
int tomo_glb_pack_faces(const int64_t *faces, int64_t nf, const uint8_t *flip, const double *volume, void *out, int out_i64,
                        void *stream);
/* POSITION: verts (nv x 3, float32 or float64) -> float32 pos (4-byte aligned), and minmax[6] = per-column min then max of
 * pos, reduced exactly in float32 (glTF requires min / max on POSITION). */
int tomo_glb_pack_positions(const void *verts, int is_f64, int64_t nv, float *pos, float *minmax, void *stream);
/* The normals contract.  pos: float32 (nv, 3); idx: the oriented faces (nf, 3), uint32 or (idx_i64) int64; normals: float32
 * (nv, 3), 4-byte aligned (the NORMAL block of the chunk).  counters[2] (zeroed by the call): [0] vertices that got the
 * default (0, 0, 1), [1] faces with an index outside [0, nv) -- they enter no sum and nothing is read through them; the mesh
 * is invalid when this is not 0.  No float atomics: an inverted index (per vertex the faces that name it: integer atomics
 * count and fill it, tomo_mc_scan places the lists), and one lane per vertex brings its list into ascending order -- in
 * registers up to 16 entries, by repeated selection across the wave beyond -- and sums.  workspace: 256-byte aligned,
 * tomo_mesh_vertex_normals_workspace_bytes(nv, nf) bytes (about 8 nv + 12 nf); nv < 2^32 - 1 and 3 nf < 2^32
 * (TOMO_E_SIZE otherwise). */
int64_t tomo_mesh_vertex_normals_workspace_bytes(int64_t nv, int64_t nf);
int tomo_mesh_vertex_normals(const float *pos, int64_t nv, const void *idx, int idx_i64, int64_t nf, void *workspace,
                             int64_t workspace_bytes, float *normals, unsigned long long *counters, void *stream);

/* tomo_mesh_vertex_normals for one rank of a multi-rank mesh: nv = own rows followed by n_raw ghost rows, idx in these local
 * numbers, nf >= 0.  The first n_seed vertices start their sums from seed (float64 (n_seed, 3)) instead of +0.0; the last
 * n_raw vertices get no normal: their raw float64 sums go to raw ((n_raw, 3)) and they are not counted.  Both the register
 * path and the long-list path honour the seed.  normals: float32 (nv - n_raw, 3).  phase 1: build the lists in the
 * workspace, zero the counters, write raw; phase 2: the normals, from the lists phase 1 left in the same workspace (same nv,
 * nf); 3: both.  Between the two a rank sends raw up and receives its seed.  Workspace as for tomo_mesh_vertex_normals
 * (sized with max(nf, 1)).  With n_seed = n_raw = 0 and phase 3 it is tomo_mesh_vertex_normals. */
int tomo_mesh_vertex_normals_seeded(const float *pos, int64_t nv, const void *idx, int idx_i64, int64_t nf, void *workspace,
                                    int64_t workspace_bytes, float *normals, unsigned long long *counters, const double *seed,
                                    int64_t n_seed, double *raw, int64_t n_raw, int phase, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TOMO_HIP_H */
