/* splatco_mesh.h -- C-ABI of the mesh clean-up that follows the TSDF extraction (gfx950): connected components, the size
 * filter and vertex normals of an indexed triangle mesh.  A family of its own next to splatco_raster.h, splatco_bilagrid.h,
 * splatco_normals.h and splatco_tsdf.h.
 *
 * The functions live in the same libsplatco_raster.so and report through the same scr_last_error() (splatco_raster.h), but
 * they are versioned on their own: SCR_MESH_ABI_VERSION changes when one of THESE prototypes or definitions changes, and no
 * other version does.  Every streamed function takes the stream last; every pointer is a device address except the stream
 * and the ones named *_host.  A refused call returns 1, launches nothing and leaves "name: ..." in scr_last_error().
 *
 * Mesh.  vertices [nv, 3] float32, faces [nf, 3] int32, optionally colours [nv, 3] float32, all contiguous; 0 <= nv < 2^31,
 * 3 nf < 2^31.  EVERY face index must lie in [0, nv): the kernels index with them and cannot refuse them; the caller checks
 * (splatco_amd/mesh.py: one aminmax and one host read before anything is launched).  Degenerate faces (an index twice or
 * three times) are legal and count as faces.
 *
 * Components.  Two vertices are connected when some face contains both (VERTEX connectivity: two shells that touch in one
 * vertex are one component; Open3D's cluster_connected_triangles clusters by shared EDGES and calls them two).
 *   labels[v]       int32 [nv]: the smallest vertex index of v's component; a vertex that no face references is a component
 *                   of its own
 *   vertex_faces[v] int32 [nv]: for v with labels[v] == v the number of faces whose FIRST index lies in v's component (0 for
 *                   an unreferenced vertex), 0 for every other v
 *   roots[c]        int32 [nc]: the vertices with labels[v] == v in ascending order
 *   face_counts[c]  int32 [nc]: vertex_faces[roots[c]]
 * Every output is an integer that the definition fixes uniquely: the same bits run after run, whatever the kernels do.
 * scr_mesh_components launches init (parent[v] = v, vertex_faces = 0, status = 0), hook (one thread per face unions (f0, f1)
 * and (f1, f2): both roots are found and the larger is linked under the smaller by compare-and-swap), flatten (labels[v] =
 * root of v) and the face count (integer atomic adds: order-free).  parent [nv] int32 is scratch, taken uninitialised.  Every
 * loop is bounded (a budget of 4 nv + 1024 steps per union, nv + 1 per flatten walk); a thread that runs out raises *status
 * and leaves.  scr_mesh_roots_plan brings the status to the host in bit 31 of the count it reads anyway and refuses with
 * "iteration bound" when it is set.
 *
 * Size filter.  A component is kept when its face count is >= threshold, threshold >= 1 (the caller derives it: max(1,
 * min_faces, the keep_largest-th largest face count)); a vertex is kept when vertex_faces[labels[v]] >= threshold, a face when
 * its first index is kept (then all three are).  Kept vertices and faces keep their relative order; positions and colours
 * are copied bit for bit; remap[v] is the new index of a kept vertex (undefined for a dropped one) and the kept faces are
 * written as remap[f_i].  An unreferenced vertex has count 0 and is always dropped: the output is welded, none unused.
 *
 * Three order-preserving compactions (compact.h: count, scan, write), each a *_plan that reads ONE count back to the host and
 * a *_run that writes: the roots over nv items, the kept vertices over nv items, the kept faces over nf items.  scratch:
 * scr_mesh_scratch_bytes(nv, nf) bytes, taken uninitialised, the same block for a plan and its run; it may be reused for the
 * next compaction after a run.  A run with nothing kept is a no-op.
 *
 * Vertex normals.  For vertex v: the sum, over the faces that contain v in ASCENDING face index (a face that contains v twice
 * is added once), of c = (p1 - p0) x (p2 - p0) with u = p1 - p0, w = p2 - p0, c.x = u.y w.z - u.z w.y, c.y = u.z w.x - u.x w.z,
 * c.z = u.x w.y - u.y w.x: the area-weighted face normal, un-normalised.  Everything is binary64, in the written order,
 * uncontracted (every product and every difference rounded on its own); the sum starts at +0 and adds x, y, z each on its own.
 * Then n = sum / sqrt((x x + y y) + z z), each component divided on its own and rounded to float32 once.  If the sum is zero
 * or not finite, the norm is zero or not finite, or the vertex has no face: exactly (+0, +0, +0).  No atomics, no saved state.
 * keys [3 nf] int64, ascending: v nf + f for every (face f, distinct index v of f), and the value nv nf (or larger) in the
 * slots that within-face duplicates leave over.  One thread per vertex finds its first key by binary search and walks its run.
 */
#ifndef SPLATCO_MESH_H
#define SPLATCO_MESH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCR_MESH_ABI_VERSION 1

int scr_mesh_abi_version(void);
size_t scr_mesh_scratch_bytes(int64_t nv, int64_t nf);
int scr_mesh_components(int64_t nv, int64_t nf, const int32_t* faces, int32_t* parent, int32_t* labels, int32_t* vertex_faces,
                        int32_t* status, void* stream);
int scr_mesh_roots_plan(int64_t nv, const int32_t* labels, const int32_t* status, void* scratch, int64_t* count_host, void* stream);
int scr_mesh_roots_run(int64_t nv, const int32_t* labels, const int32_t* vertex_faces, const void* scratch, int64_t nc,
                       int32_t* roots, int32_t* face_counts, void* stream);
int scr_mesh_vertices_plan(int64_t nv, const int32_t* labels, const int32_t* vertex_faces, int32_t threshold, void* scratch,
                           int64_t* count_host, void* stream);
int scr_mesh_vertices_run(int64_t nv, const int32_t* labels, const int32_t* vertex_faces, int32_t threshold, const void* scratch,
                          int64_t nkept, const float* vertices, const float* colors, float* out_vertices, float* out_colors,
                          int32_t* remap, void* stream);
int scr_mesh_faces_plan(int64_t nf, const int32_t* faces, const int32_t* labels, const int32_t* vertex_faces, int32_t threshold,
                        void* scratch, int64_t* count_host, void* stream);
int scr_mesh_faces_run(int64_t nf, const int32_t* faces, const int32_t* labels, const int32_t* vertex_faces, int32_t threshold,
                       const void* scratch, int64_t nkept, const int32_t* remap, int32_t* out_faces, void* stream);
int scr_mesh_vertex_normals(int64_t nv, int64_t nf, const float* vertices, const int32_t* faces, const int64_t* keys,
                            float* normals, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPLATCO_MESH_H */
