/* splatco_tsdf_sparse.h -- C-ABI of the block-sparse TSDF volume (gfx950): the fusion and the mesh extraction of splatco_tsdf.h
 * on a volume that stores 8 x 8 x 8-node blocks only where a depth map puts a surface.  A family of its own: the functions live
 * in the same libsplatco_raster.so and report through the same scr_last_error(), but SCR_TSDFS_ABI_VERSION changes only when
 * one of THESE prototypes or definitions changes.  Every streamed function takes the stream last; every pointer is a device
 * address except the stream and the ones named *_host.  A refused call returns 1, launches nothing and leaves "name: ..." in
 * scr_last_error(); scalars are checked first and pointers last.
 *
 * Virtual lattice.  lo, h, dims = (nx, ny, nz), trunc and max_weight are splatco_tsdf.h's: node p(i, j, k) = lo + h (i, j, k).
 * Every dimension is >= 2 and < 2^20; the node count may exceed 2^31.  Blocks have B = 8 nodes per side, nb? = ceil(n? / 8);
 * block (bi, bj, bk) has the key (bk nby + bj) nbx + bi, an int32: nbx nby nbz < 2^31.  A node's local index in its block is
 * l = (lk 8 + lj) 8 + li.  Nodes of an edge block that lie outside dims exist in storage, are never updated (weight 0) and
 * belong to no cube.
 *
 * Storage.  keys [Nb] int32 ascending; slots [Nb] int32, the storage row of each key; tsdf [cap, 512] and weight [cap, 512]
 * float32, colour [cap, 3, 512] float32 or NULL; marks [nbx nby nbz] uint8, one per virtual block: 0 untouched, 1 touched by
 * a view but not allocated, 2 allocated.  A new block holds tsdf 1, weight 0, colour 0 (scr_tsdfs_init_blocks).  Storage rows
 * are given in allocation order: the new blocks of one allocation take the rows Nb_old + rank, rank their position among the
 * new keys in ascending order.  Growing the capacity (the caller's) copies rows and changes no bit.
 *
 * Allocation for one view (struct scr_tsdfs_view: the scr_tsdf_view and c2w, the first three ROWS of the binary64 inverse of
 * the 4 x 4 world-to-camera matrix, computed by the host).  For every pixel (px, py) that passes step 3 of splatco_tsdf.h:
 *   1. z = (double)(float)(D / A), z0 = max(z - trunc, near), z1 = z + trunc;  if z0 > z1 the pixel allocates nothing
 *   2. the 8 camera-space corners ((px + dx - cx) / fx zc, (py + dy - cy) / fy zc, zc), dx, dy in {0, 1}, zc in {z0, z1}
 *   3. moved to world space, each row ((c0 x + c1 y) + c2 z) + c3 of c2w
 *   4. their axis-aligned box, padded by h / 8 on every side
 *   5. block ranges floor((min - lo) / (8 h)) .. floor((max - lo) / (8 h)) per axis, clipped to the grid; an empty range
 *      allocates nothing
 *   6. every block of the range that is not yet allocated is allocated
 * All arithmetic binary64.  A node whose projection floors to (px, py) with zc in [z0, z1] lies inside that frustum slab, which
 * is convex, so every node the dense update moves with |sdf| <= trunc is covered; free space in front of the band (d = 1) is
 * deliberately not allocated.  scr_tsdfs_alloc_plan marks the touched blocks (plain same-value stores of 1 over 0: the
 * result does not depend on timing), counts the marks that are 1 by a compaction over the virtual blocks and reads that ONE
 * count to the host; scr_tsdfs_alloc_run writes the marked keys in ascending order to new_keys, sets their marks to 2 and merges
 * them with the old lists into keys / slots [nb_old + nnew] (fresh arrays; the old ones are only read).  A plan whose run is
 * not made leaves marks of 1 behind; the caller clears them or they join the next allocation.
 *
 * Integration of one view: every allocated block is visited, and every node of it that lies inside dims gets steps 1 to 5 of
 * splatco_tsdf.h with p taken from its virtual integer coordinates -- the same device code as scr_tsdf_integrate, hence the
 * same bits.  No atomics, one owner per node, one view per launch.  A block all of whose nodes are behind `near`, or outside
 * the image on one side, is left early; the test is made on bounds of the very floating-point values the nodes would compute
 * (every step of them is monotone in each lattice coordinate), so it changes no bit.
 * ORDER DEPENDENCE, inherent: a block allocated at view a has missed the views before a; its nodes hold what a dense volume
 * fused from the views a, a + 1, ... holds.  Allocating for all views first and integrating them afterwards gives exactly the
 * dense volume on every allocated block.
 *
 * Extraction: the marching tetrahedra of splatco_tsdf.h (Kuhn tetrahedra, inside test, vertex formula with a the edge's own
 * node, triangle tables, winding).  A cube is valid when its corner is in an allocated block, all 8 of its nodes lie inside
 * dims and in allocated blocks, and all have weight > min_weight.  An edge belongs to the block of its own (lower) node, local
 * id 7 l + dir; the cubes around it may have their corner in any of the 26 neighbour blocks, found through table [Nb, 27]
 * int32 (scr_tsdfs_neighbors, binary search in keys, once per extraction): entry ((dk + 1) 3 + (dj + 1)) 3 + (di + 1) of
 * row r is the RANK in keys of the block at offset (di, dj, dk) from block keys[r], or -1; its storage row is slots[rank], and
 * the rank is also what edge ids are made of.  There is no dense block map.  Vertices come in ascending (block key, local edge
 * id), faces in ascending (block key, local cube l, tetrahedron q, triangle); the mesh is indexed and welded, int32 indices,
 * Nv, Nf < 2^31.  Two order-preserving compactions (compact.h), each a *_plan with ONE host read and a *_run: over the 3584 Nb
 * edge ids and over the 6144 Nb triangle slots.  A pass covers the blocks of rank first .. first + count - 1, 6144 count < 2^31
 * (count <= 349525): a volume of that many blocks is ONE pass (first = 0, count = Nb) and one host read per compaction; a larger
 * one is cut into passes in rank order by the caller, which first runs every vertex pass (each writes its own nv kept ids,
 * vertices and colours; joined in pass order they are the volume's lists) and then every face pass, whose run is handed the
 * JOINED edge_ids and their number nv and writes its own nf faces.  scratch: scr_tsdfs_extract_scratch_bytes(count) bytes, taken
 * uninitialised, the same block for a plan and its run.  edge_ids int64 holds the kept ids 3584 r + 7 l + dir, r the block's
 * rank in keys: sorted by construction, and faces find them by binary search.  A run with nv or nf == 0 is a no-op.
 */
#ifndef SPLATCO_TSDF_SPARSE_H
#define SPLATCO_TSDF_SPARSE_H

#include <stddef.h>
#include <stdint.h>

#include "splatco_tsdf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCR_TSDFS_ABI_VERSION 1
#define SCR_TSDFS_BLOCK 8

typedef struct scr_tsdfs_view {
    scr_tsdf_view view;
    double c2w[12];
} scr_tsdfs_view;

int scr_tsdfs_abi_version(void);
size_t scr_tsdfs_alloc_scratch_bytes(int32_t nx, int32_t ny, int32_t nz);
int scr_tsdfs_alloc_plan(int32_t nx, int32_t ny, int32_t nz, const float* lo_host, float h, double trunc,
                         const scr_tsdfs_view* view_host, uint8_t* marks, void* scratch, int64_t* count_host, void* stream);
int scr_tsdfs_alloc_run(int32_t nx, int32_t ny, int32_t nz, uint8_t* marks, const void* scratch, int64_t nb_old,
                        const int32_t* keys_old, const int32_t* slots_old, int64_t nnew, int32_t* new_keys, int32_t* keys,
                        int32_t* slots, void* stream);
int scr_tsdfs_init_blocks(int64_t first, int64_t count, float* tsdf, float* weight, float* color, void* stream);
int scr_tsdfs_integrate(int32_t nx, int32_t ny, int32_t nz, const float* lo_host, float h, double trunc, float max_weight, int64_t nb,
                        const int32_t* keys, const int32_t* slots, float* tsdf, float* weight, float* color,
                        const scr_tsdfs_view* view_host, void* stream);
int scr_tsdfs_neighbors(int32_t nx, int32_t ny, int32_t nz, int64_t nb, const int32_t* keys, int32_t* table, void* stream);
size_t scr_tsdfs_extract_scratch_bytes(int64_t count);
int scr_tsdfs_extract_vertices_plan(int32_t nx, int32_t ny, int32_t nz, int64_t nb, int64_t first, int64_t count, const int32_t* keys,
                                    const int32_t* slots, const int32_t* table, const float* tsdf, const float* weight,
                                    float min_weight, void* scratch, int64_t* count_host, void* stream);
int scr_tsdfs_extract_vertices_run(int32_t nx, int32_t ny, int32_t nz, const float* lo_host, float h, int64_t nb, int64_t first,
                                   int64_t count, const int32_t* keys, const int32_t* slots, const int32_t* table, const float* tsdf,
                                   const float* weight, const float* color, float min_weight, const void* scratch, int64_t nv,
                                   int64_t* edge_ids, float* vertices, float* colors, void* stream);
int scr_tsdfs_extract_faces_plan(int32_t nx, int32_t ny, int32_t nz, int64_t nb, int64_t first, int64_t count, const int32_t* keys,
                                 const int32_t* slots, const int32_t* table, const float* tsdf, const float* weight, float min_weight,
                                 void* scratch, int64_t* count_host, void* stream);
int scr_tsdfs_extract_faces_run(int32_t nx, int32_t ny, int32_t nz, int64_t nb, int64_t first, int64_t count, const int32_t* keys,
                                const int32_t* slots, const int32_t* table, const float* tsdf, const float* weight, float min_weight,
                                const void* scratch, int64_t nv, const int64_t* edge_ids, int64_t nf, int32_t* faces, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPLATCO_TSDF_SPARSE_H */
