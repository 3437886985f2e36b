// rtk_refit.hip -- new vertex positions for a finished device scene, in place (rtk_dev_scene_refit).
//
// The tree stays: slots, primitive ids, node numbers, child words, depth. What depends on positions is made again:
//   k_refit_tris    the 36 position bytes of every 48-byte triangle record, gathered through the vertex indices the scene
//                   recorded (view.vertex_index), prim / flags / spare kept;
//   k_refit_level   the child boxes of every node, bottom-up BY HEIGHT: a node's height is 0 if none of its children is an
//   k_refit_small   inner node, else 1 + the largest height among them, so every inner child of a node of height h was
//                   written by the launch of a lower height. One launch per height while a height has many nodes; the
//                   heights near the root (a few hundred nodes over a dozen heights) share ONE launch of one workgroup
//                   with a barrier between heights. Visibility between launches comes from the kernel boundary alone
//                   (the XCD L2s are not coherent; a counter per node climbing inside one launch would need an
//                   agent-scope release and acquire per hand-off);
//   k_quantize      (rtk_quant.hip) the 64-byte compressed nodes, the child order words and the scene constants.
// The heights and the node numbers grouped by them (RefitSchedule) are made by the first refit of a scene and kept.
// A box is made by the validator's rule (rtk_validate.hip: fminf / fmaxf over the vertices of a leaf, over the non-empty
// slots of an inner child), so after a refit every box is the exact union of what is below it.
#include "rtk_dev.h"

#include <math.h>
#include <string.h>

#include <chrono>
#include <vector>

namespace {

// where one mesh's positions are read from (device memory: the caller's own buffer or its copy in the workspace)
struct RefitMesh {
	const char *pos;
	unsigned long long stride;
	uint32_t f64;
	uint32_t pad;
};
static_assert(sizeof(RefitMesh) == 24, "RefitMesh");

#define REFIT_SMALL_THREADS 1024                 // k_refit_small: four lanes per node, 256 nodes per trip
#define REFIT_SMALL_LEVEL 1024u                // heights of at most this many nodes go to k_refit_small

// ---------------------------------------------------------------------------------- schedule (once per scene)

// One Jacobi sweep of height[i] = max over inner children (height[child] + 1). Heights only grow and a stale read is a
// lower bound, so the sweeps converge whatever a launch sees of its own stores: after sweep k every node of height < k is
// final (the kernel boundary makes sweep k - 1 visible).
__global__ void k_refit_heights(const DevNode *nodes, uint32_t n, uint32_t *height, uint32_t *changed)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint4 c = *reinterpret_cast<const uint4 *>(nodes[i].child);
	const uint32_t ref[4] = { c.x, c.y, c.z, c.w };
	uint32_t h = 0;
	for (int k = 0; k < 4; k++) {
		if (ref[k] == RTK_REF_NONE || (ref[k] & RTK_REF_LEAF) || ref[k] >= n) continue;
		const uint32_t hc = height[ref[k]] + 1u;
		h = hc > h ? hc : h;
	}
	if (h > height[i]) { height[i] = h; *changed = 1u; }
}

__global__ void k_refit_keys(const uint32_t *height, uint32_t n, unsigned long long *keys)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) keys[i] = ((unsigned long long)height[i] << 32) | i;
}

// sorted (height, node) words -> the node numbers, and where each height begins (every height up to the largest occurs: a
// node of height h has a child of height h - 1)
__global__ void k_refit_order(const unsigned long long *keys, uint32_t n, uint32_t *order, uint32_t *level_start)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const unsigned long long k = keys[i];
	const uint32_t h = (uint32_t)(k >> 32);
	order[i] = (uint32_t)k;
	if (i == 0u || (uint32_t)(keys[i - 1u] >> 32) != h) level_start[h] = i;
	if (i == n - 1u) level_start[h + 1u] = n;
}

// the largest vertex index each mesh's triangles use (how far a host-resident position buffer has to be copied)
__global__ void k_refit_max_vertex(const uint32_t *vertex_index, const uint32_t *slot_mesh, uint32_t n, uint32_t num_meshes, uint32_t *max_vertex)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	uint32_t mesh = 0xffffffffu, v = 0;
	if (s < n) {
		mesh = slot_mesh[s];
		const uint32_t a = vertex_index[3 * (size_t)s], b = vertex_index[3 * (size_t)s + 1], c = vertex_index[3 * (size_t)s + 2];
		v = a > b ? a : b;
		v = c > v ? c : v;
	}
	// slots follow the tree, so a wave is mostly inside one mesh: one atomic per wave then
	const uint32_t first = __shfl(mesh, 0);
	if (__builtin_amdgcn_ballot_w64(mesh != first) == 0ull) {
		for (int o = 32; o > 0; o >>= 1) { const uint32_t t = __shfl_xor(v, o); v = t > v ? t : v; }
		if ((threadIdx.x & 63u) == 0u && mesh < num_meshes) atomicMax(&max_vertex[mesh], v);
	} else if (mesh < num_meshes) atomicMax(&max_vertex[mesh], v);
}

// ---------------------------------------------------------------------------------- triangles

// MODE 0: every mesh has float positions, 1: every mesh doubles, 2: per mesh (RefitMesh::f64, a flag the host derived from
// validated type codes). Doubles are converted as k_ingest converts them.
template <int MODE>
__global__ void __launch_bounds__(256) k_refit_tris(DevTri *tris, uint32_t n, const uint32_t *vertex_index, const uint32_t *slot_mesh,
	const RefitMesh *meshes, uint32_t num_meshes)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s >= n) return;
	const uint32_t mesh = slot_mesh[s];
	if (mesh >= num_meshes) return;
	const RefitMesh ms = meshes[mesh];
	const uint32_t vi[3] = { vertex_index[3 * (size_t)s], vertex_index[3 * (size_t)s + 1], vertex_index[3 * (size_t)s + 2] };
	float p[3][3];
	const bool f64 = MODE == 1 || (MODE == 2 && ms.f64 != 0u);
#pragma unroll
	for (int c = 0; c < 3; c++) {
		if (f64) {
			const double *q = reinterpret_cast<const double *>(ms.pos + (size_t)vi[c] * ms.stride);
			p[c][0] = (float)q[0]; p[c][1] = (float)q[1]; p[c][2] = (float)q[2];
		} else {
			const float *q = reinterpret_cast<const float *>(ms.pos + (size_t)vi[c] * ms.stride);
			p[c][0] = q[0]; p[c][1] = q[1]; p[c][2] = q[2];
		}
	}
	// (the w lanes -- prim, flags, spare -- stay; a record is RTK_TRI_STRIDE bytes apart, 48 of them payload)
	float4 *rec = reinterpret_cast<float4 *>(tris + s);
	float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
	r0.x = p[0][0]; r0.y = p[0][1]; r0.z = p[0][2];
	r1.x = p[1][0]; r1.y = p[1][1]; r1.z = p[1][2];
	r2.x = p[2][0]; r2.y = p[2][1]; r2.z = p[2][2];
	rec[0] = r0; rec[1] = r1; rec[2] = r2;
}

// ---------------------------------------------------------------------------------- boxes

// Child slot k of `node`: its box from what is below it, stored into the node (the four lanes of a node store four
// neighbouring words each time). The child words are left alone.
__device__ __forceinline__ void refit_child(DevNode *nodes, const DevTri *tris, uint32_t num_nodes, uint32_t num_tris, uint32_t node, uint32_t k)
{
	DevNode *nd = nodes + node;
	const uint32_t ref = nd->child[k];
	float mn[3] = { 1.0f, 1.0f, 1.0f }, mx[3] = { -1.0f, -1.0f, -1.0f };         // an empty slot keeps the inverted box
	if (ref != RTK_REF_NONE) {
		// The union starts from its first member, as the build's does, and grows by fminf / fmaxf: a NaN is skipped unless
		// EVERY member is one (a leaf of all-NaN triangles gets the NaN box a build gives it, which the validator reports
		// for both); with nothing below the slot -- a broken reference -- the box is the empty union.
		bool first_member = true;
		mn[0] = mn[1] = mn[2] = INFINITY;
		mx[0] = mx[1] = mx[2] = -INFINITY;
		if (ref & RTK_REF_LEAF) {
			const uint32_t first = ref & 0x7fffffffu;
			uint32_t cnt = first < num_tris ? tris[first].spare : 0u;
			if (cnt > 63u) cnt = 63u;
			if (cnt > num_tris - first) cnt = num_tris - first;
			for (uint32_t t = 0; t < cnt; t++) {
				const float4 *rec = reinterpret_cast<const float4 *>(tris + first + t);
				const float4 a = rec[0], b = rec[1], c = rec[2];
				const float lo[3] = { fminf(fminf(a.x, b.x), c.x), fminf(fminf(a.y, b.y), c.y), fminf(fminf(a.z, b.z), c.z) };
				const float hi[3] = { fmaxf(fmaxf(a.x, b.x), c.x), fmaxf(fmaxf(a.y, b.y), c.y), fmaxf(fmaxf(a.z, b.z), c.z) };
#pragma unroll
				for (int ax = 0; ax < 3; ax++) {
					mn[ax] = first_member ? lo[ax] : fminf(mn[ax], lo[ax]);
					mx[ax] = first_member ? hi[ax] : fmaxf(mx[ax], hi[ax]);
				}
				first_member = false;
			}
		} else if (ref < num_nodes) {
			const DevNode *ch = nodes + ref;
			const float4 *w = reinterpret_cast<const float4 *>(ch);
			const float4 xl = w[0], xh = w[1], yl = w[2], yh = w[3], zl = w[4], zh = w[5];
			const uint4 cc = *reinterpret_cast<const uint4 *>(ch->child);
			const float bl[3][4] = { { xl.x, xl.y, xl.z, xl.w }, { yl.x, yl.y, yl.z, yl.w }, { zl.x, zl.y, zl.z, zl.w } };
			const float bh[3][4] = { { xh.x, xh.y, xh.z, xh.w }, { yh.x, yh.y, yh.z, yh.w }, { zh.x, zh.y, zh.z, zh.w } };
			const uint32_t cr[4] = { cc.x, cc.y, cc.z, cc.w };
#pragma unroll
			for (int q = 0; q < 4; q++) {
				if (cr[q] == RTK_REF_NONE) continue;
#pragma unroll
				for (int ax = 0; ax < 3; ax++) {
					mn[ax] = first_member ? bl[ax][q] : fminf(mn[ax], bl[ax][q]);
					mx[ax] = first_member ? bh[ax][q] : fmaxf(mx[ax], bh[ax][q]);
				}
				first_member = false;
			}
		}
	}
	nd->bx[0][k] = mn[0]; nd->bx[1][k] = mx[0];
	nd->by[0][k] = mn[1]; nd->by[1][k] = mx[1];
	nd->bz[0][k] = mn[2]; nd->bz[1][k] = mx[2];
}

// one height: entries [begin, end) of `order`, four lanes per node
__global__ void __launch_bounds__(256) k_refit_level(DevNode *nodes, const DevTri *tris, uint32_t num_nodes, uint32_t num_tris,
	const uint32_t *order, uint32_t begin, uint32_t end)
{
	const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t e = begin + (t >> 2);
	if (e >= end) return;
	const uint32_t node = order[e];
	if (node < num_nodes) refit_child(nodes, tris, num_nodes, num_tris, node, t & 3u);
}

// heights [h0, h1) in one workgroup: what a height stores is read by the next one behind a barrier (workgroup scope is all
// that is needed: one workgroup; the kernel boundary does the rest)
__global__ void __launch_bounds__(REFIT_SMALL_THREADS) k_refit_small(DevNode *nodes, const DevTri *tris, uint32_t num_nodes, uint32_t num_tris,
	const uint32_t *order, const uint32_t *level_start, uint32_t h0, uint32_t h1)
{
	for (uint32_t h = h0; h < h1; h++) {
		const uint32_t begin = level_start[h], end = level_start[h + 1u];
		for (uint32_t e = begin + (threadIdx.x >> 2); e < end; e += REFIT_SMALL_THREADS / 4) {
			const uint32_t node = order[e];
			if (node < num_nodes) refit_child(nodes, tris, num_nodes, num_tris, node, threadIdx.x & 3u);
		}
		__syncthreads();
	}
}

// ---------------------------------------------------------------------------------- host

#define REFIT_CHECK(expr)                                                                                    \
	do {                                                                                                     \
		hipError_t e_ = (expr);                                                                              \
		if (e_ != hipSuccess) {                                                                              \
			rtk_set_error("rtk_dev_scene_refit: %s failed: %s (line %d)", #expr, hipGetErrorString(e_), __LINE__); \
			return RTK_AMD_ERR_HIP;                                                                          \
		}                                                                                                    \
	} while (0)

// temporaries of the schedule: heights, the changed word, two key arrays, the sort's scratch, level starts
struct ScheduleTmp { size_t o_changed, o_ka, o_kb, o_sort, o_ls, bytes; };
ScheduleTmp schedule_tmp(uint32_t n)
{
	ScheduleTmp t;
	t.o_changed = rtk_padded((size_t)n * 4);
	t.o_ka = t.o_changed + rtk_padded(4);
	t.o_kb = t.o_ka + rtk_padded((size_t)n * 8);
	t.o_sort = t.o_kb + rtk_padded((size_t)n * 8);
	t.o_ls = t.o_sort + rtk_padded(rtk_sort_scratch_words(n) * 4);
	t.bytes = t.o_ls + rtk_padded(((size_t)n + 2) * 4);
	return t;
}

// heights, node numbers grouped by height, the mesh table's memory: once per scene. tmp: schedule_tmp(num_nodes).bytes of
// device memory (the borrowed workspace: no allocation of a quarter of a gigabyte at 10M triangles, freed again at once)
int make_schedule(rtk_dev_scene *ds, hipStream_t stream, char *tmp)
{
	RefitSchedule &rs = ds->refit;
	if (rs.ready) return RTK_AMD_OK;
	const uint32_t n = ds->view.num_nodes;
	const size_t num_meshes = ds->mesh_base.empty() ? 0 : ds->mesh_base.size() - 1;
	const ScheduleTmp T = schedule_tmp(n);
	uint32_t *d_height = (uint32_t *)tmp, *d_changed = (uint32_t *)(tmp + T.o_changed), *d_ls = (uint32_t *)(tmp + T.o_ls);
	unsigned long long *keys_a = (unsigned long long *)(tmp + T.o_ka), *keys_b = (unsigned long long *)(tmp + T.o_kb);
	void *d_order = nullptr, *d_small = nullptr;
	int rc = RTK_AMD_OK;
	std::vector<uint32_t> level_start;
	do {
#define SCHED_CHECK(expr) if ((expr) != hipSuccess) { rtk_set_error("rtk_dev_scene_refit: schedule: %s failed: %s", #expr, hipGetErrorString(hipGetLastError())); rc = RTK_AMD_ERR_HIP; break; }
		const unsigned blocks = (n + 255u) / 256u;
		SCHED_CHECK(hipMemsetAsync(d_height, 0, (size_t)n * 4, stream));
		// A tree has no cycle and its heights are below max_depth, so max_depth sweeps settle them; one more, which must change
		// nothing, is the proof, and the one wait of the host. (Should a scene's max_depth be too small the rounds go on, eight
		// sweeps at a time.)
		uint32_t sweeps = 0, round = ds->max_depth < 4096u ? ds->max_depth + 1u : 4096u;
		bool converged = false;
		while (!converged && rc == RTK_AMD_OK) {
			uint32_t h_changed = 0;
			for (uint32_t k = 0; k + 1u < round; k++) hipLaunchKernelGGL(k_refit_heights, dim3(blocks), dim3(256), 0, stream, ds->view.nodes, n, d_height, d_changed);
			if (hipMemsetAsync(d_changed, 0, 4, stream) != hipSuccess) { rc = RTK_AMD_ERR_HIP; break; }
			hipLaunchKernelGGL(k_refit_heights, dim3(blocks), dim3(256), 0, stream, ds->view.nodes, n, d_height, d_changed);
			sweeps += round;
			round = 8u;
			if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&h_changed, d_changed, 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
				hipStreamSynchronize(stream) != hipSuccess) { rc = RTK_AMD_ERR_HIP; break; }
			converged = h_changed == 0u;
			if (!converged && sweeps > n + 8u) { rc = RTK_AMD_ERR_BAD_SCENE; break; }
		}
		if (rc != RTK_AMD_OK) { rtk_set_error("rtk_dev_scene_refit: schedule: heights did not settle (%s)", rc == RTK_AMD_ERR_HIP ? hipGetErrorString(hipGetLastError()) : "not a tree"); break; }
		hipLaunchKernelGGL(k_refit_keys, dim3(blocks), dim3(256), 0, stream, d_height, n, keys_a);
		// heights are below n: that many bits of the upper word, in whole 8-bit passes; stable, so numbers stay in order
		const unsigned long long bound = n;
		uint32_t bits = 1;
		while (bits < 32u && (1ull << bits) <= bound) bits++;
		const unsigned long long *sorted = keys_a;
		if (n > 1u) sorted = rtk_sort_words_async(keys_a, keys_b, n, 32u, 32u + bits, (uint32_t *)(tmp + T.o_sort), stream) ? keys_b : keys_a;
		SCHED_CHECK(hipMalloc(&d_order, (size_t)n * 4));
		hipLaunchKernelGGL(k_refit_order, dim3(blocks), dim3(256), 0, stream, sorted, n, (uint32_t *)d_order, d_ls);
		unsigned long long last = 0;
		SCHED_CHECK(hipGetLastError());
		SCHED_CHECK(hipMemcpyAsync(&last, sorted + (n - 1u), 8, hipMemcpyDeviceToHost, stream));
		SCHED_CHECK(hipStreamSynchronize(stream));
		const uint32_t heights = (uint32_t)(last >> 32) + 1u;
		if (heights > n) { rtk_set_error("rtk_dev_scene_refit: schedule: %u heights for %u nodes", heights, n); rc = RTK_AMD_ERR_BAD_SCENE; break; }
		level_start.resize((size_t)heights + 1);
		SCHED_CHECK(hipMemcpy(level_start.data(), d_ls, level_start.size() * 4, hipMemcpyDeviceToHost));
		bool sane = level_start.front() == 0u && level_start.back() == n;
		for (size_t h = 0; h + 1 < level_start.size(); h++) sane = sane && level_start[h] < level_start[h + 1];
		if (!sane) { rtk_set_error("rtk_dev_scene_refit: schedule: heights are not contiguous"); rc = RTK_AMD_ERR_BAD_SCENE; break; }
		// the level starts and the mesh table share one small allocation
		const size_t o_meshes = rtk_padded(level_start.size() * 4);
		SCHED_CHECK(hipMalloc(&d_small, o_meshes + (num_meshes ? num_meshes : 1) * sizeof(RefitMesh)));
		SCHED_CHECK(hipMemcpy(d_small, level_start.data(), level_start.size() * 4, hipMemcpyHostToDevice));
		rs.d_meshes = (char *)d_small + o_meshes;
#undef SCHED_CHECK
	} while (0);
	if (rc != RTK_AMD_OK) {
		if (d_order) (void)hipFree(d_order);
		if (d_small) (void)hipFree(d_small);
		rs.d_meshes = nullptr;
		return rc;
	}
	ds->allocs.push_back(d_order); ds->allocs.push_back(d_small);
	ds->total_bytes += (size_t)n * 4 + level_start.size() * 4 + num_meshes * sizeof(RefitMesh);
	rs.d_order = (uint32_t *)d_order;
	rs.d_level_start = (uint32_t *)d_small;
	rs.level_start.swap(level_start);
	rs.ready = true;
	return RTK_AMD_OK;
}

int make_max_vertex(rtk_dev_scene *ds, hipStream_t stream)
{
	RefitSchedule &rs = ds->refit;
	if (rs.max_vertex_ready) return RTK_AMD_OK;
	const size_t num_meshes = ds->mesh_base.size() - 1;
	const uint32_t n = ds->view.num_tris;
	std::vector<uint32_t> mv(num_meshes, 0u);
	if (n) {
		uint32_t *d = nullptr;
		if (hipMalloc(&d, num_meshes * 4) != hipSuccess) { (void)hipGetLastError(); rtk_set_error("rtk_dev_scene_refit: out of device memory"); return RTK_AMD_ERR_OOM; }
		bool ok = hipMemsetAsync(d, 0, num_meshes * 4, stream) == hipSuccess;
		if (ok) hipLaunchKernelGGL(k_refit_max_vertex, dim3((n + 255u) / 256u), dim3(256), 0, stream, ds->view.vertex_index, ds->view.slot_mesh, n, (uint32_t)num_meshes, d);
		ok = ok && hipGetLastError() == hipSuccess && hipMemcpyAsync(mv.data(), d, num_meshes * 4, hipMemcpyDeviceToHost, stream) == hipSuccess &&
			hipStreamSynchronize(stream) == hipSuccess;
		(void)hipFree(d);
		if (!ok) { rtk_set_error("rtk_dev_scene_refit: %s", hipGetErrorString(hipGetLastError())); return RTK_AMD_ERR_HIP; }
	}
	rs.max_vertex.swap(mv);
	rs.max_vertex_ready = true;
	return RTK_AMD_OK;
}

// everything behind the argument checks; the scene's device is current
int refit_on_device(rtk_dev_scene *ds, const rtk_scene_desc *desc, hipStream_t stream, WorkspaceLoan &loan)
{
	int rc = rtk_scene_side_arrays(ds, stream);
	if (rc != RTK_AMD_OK) return rc;
	RefitSchedule &rs = ds->refit;
	if (ds->view.num_nodes == 0u) { rtk_set_error("rtk_dev_scene_refit: scene without a root node"); return RTK_AMD_ERR_BAD_SCENE; }
	const DevSceneView &v = ds->view;
	const size_t num_meshes = desc->num_meshes;

	// ---- where every mesh's positions are read from
	std::vector<RefitMesh> table(num_meshes ? num_meshes : 1, RefitMesh{ nullptr, 0ull, 0u, 0u });
	std::vector<size_t> upload(num_meshes, 0);
	size_t upload_bytes = 0;
	bool any_device = false, any_f32 = false, any_f64 = false;
	for (size_t mi = 0; mi < num_meshes; mi++) {
		const rtk_mesh *m = &desc->meshes[mi];
		if (m->num_triangles == 0) continue;
		RefitMesh &t = table[mi];
		t.f64 = m->position.type == RTK_TYPE_F64 ? 1u : 0u;
		t.stride = m->position.stride ? m->position.stride : (t.f64 ? 24 : 12);
		t.pos = (const char *)m->position.data;
		(t.f64 ? any_f64 : any_f32) = true;
		if (rtk_is_device_ptr(m->position.data)) { any_device = true; continue; }
		rc = make_max_vertex(ds, stream);
		if (rc != RTK_AMD_OK) return rc;
		upload[mi] = (size_t)rs.max_vertex[mi] * t.stride + (t.f64 ? 24 : 12);
		upload_bytes += rtk_padded(upload[mi]);
	}
	// the workspace: first the temporaries of the schedule (the first refit of a scene; over when make_schedule returns), then
	// the staged positions
	const size_t schedule_bytes = rs.ready ? 0 : schedule_tmp(ds->view.num_nodes).bytes;
	const size_t borrow = schedule_bytes > upload_bytes ? schedule_bytes : upload_bytes;
	if (borrow && !loan.take(ds->device, borrow)) return RTK_AMD_ERR_OOM;
	rc = make_schedule(ds, stream, loan.base);
	if (rc != RTK_AMD_OK) return rc;
	if (upload_bytes) {
		char *base = loan.base;
		size_t off = 0;
		for (size_t mi = 0; mi < num_meshes; mi++) {
			if (!upload[mi]) continue;
			REFIT_CHECK(hipMemcpyAsync(base + off, table[mi].pos, upload[mi], hipMemcpyHostToDevice, stream));
			table[mi].pos = base + off;
			off += rtk_padded(upload[mi]);
		}
	}
	// a mesh in device memory was written by the caller's own work, possibly still in flight on the NULL stream (as in a build)
	if (any_device && stream != nullptr) REFIT_CHECK(hipStreamSynchronize(nullptr));
	if (num_meshes) REFIT_CHECK(hipMemcpyAsync(rs.d_meshes, table.data(), num_meshes * sizeof(RefitMesh), hipMemcpyHostToDevice, stream));

	// ---- triangles
	DevTri *tris = const_cast<DevTri *>(v.tris);
	DevNode *nodes = const_cast<DevNode *>(v.nodes);
	if (v.num_tris) {
		const dim3 grid((v.num_tris + 255u) / 256u), block(256);
		const RefitMesh *dm = (const RefitMesh *)rs.d_meshes;
		if (any_f64 && any_f32) hipLaunchKernelGGL((k_refit_tris<2>), grid, block, 0, stream, tris, v.num_tris, v.vertex_index, v.slot_mesh, dm, (uint32_t)num_meshes);
		else if (any_f64) hipLaunchKernelGGL((k_refit_tris<1>), grid, block, 0, stream, tris, v.num_tris, v.vertex_index, v.slot_mesh, dm, (uint32_t)num_meshes);
		else hipLaunchKernelGGL((k_refit_tris<0>), grid, block, 0, stream, tris, v.num_tris, v.vertex_index, v.slot_mesh, dm, (uint32_t)num_meshes);
		REFIT_CHECK(hipGetLastError());
	}

	// ---- boxes, height by height; runs of small heights share one launch of one workgroup
	const uint32_t heights = (uint32_t)rs.level_start.size() - 1u;
	for (uint32_t h = 0; h < heights;) {
		const uint32_t begin = rs.level_start[h], end = rs.level_start[h + 1];
		if (end - begin > REFIT_SMALL_LEVEL) {
			const unsigned blocks = (unsigned)(((size_t)(end - begin) * 4 + 255) / 256);
			hipLaunchKernelGGL(k_refit_level, dim3(blocks), dim3(256), 0, stream, nodes, tris, v.num_nodes, v.num_tris, rs.d_order, begin, end);
			h++;
		} else {
			uint32_t h1 = h + 1;
			while (h1 < heights && rs.level_start[h1 + 1] - rs.level_start[h1] <= REFIT_SMALL_LEVEL) h1++;
			hipLaunchKernelGGL(k_refit_small, dim3(1), dim3(REFIT_SMALL_THREADS), 0, stream, nodes, tris, v.num_nodes, v.num_tris, rs.d_order, rs.d_level_start, h, h1);
			h = h1;
		}
	}
	REFIT_CHECK(hipGetLastError());

	// ---- compressed nodes, order words, constants (the block is cleared first: the misfit count starts at zero); every box
	// lies inside the root's now, so no bound is passed in
	rc = rtk_quantize_nodes(ds, stream, nullptr, const_cast<DevNodeQ *>(ds->qnodes_mem), 0.0f, 0xffffffffu, false, true);
	if (rc != RTK_AMD_OK) return rc;
	REFIT_CHECK(hipStreamSynchronize(stream));
	{
		// (the trace path reads these host fields under the same mutex when it enqueues a launch)
		std::lock_guard<std::mutex> lock(ds->scratch_mutex);
		rtk_quantize_finish(ds);
	}
	rtk_export_forget(ds);
	return RTK_AMD_OK;
}

} // namespace

extern "C" int rtk_dev_scene_refit(rtk_dev_scene *ds, const rtk_scene_desc *desc, void *stream)
{
	// ---- everything that can be refused is refused here, before HIP is touched
	if (!ds || !desc) { rtk_set_error("rtk_dev_scene_refit: NULL argument"); return RTK_AMD_ERR_BAD_ARG; }
	if (!desc->meshes && desc->num_meshes) { rtk_set_error("rtk_dev_scene_refit: NULL meshes"); return RTK_AMD_ERR_BAD_ARG; }
	const size_t scene_meshes = ds->mesh_base.empty() ? 0 : ds->mesh_base.size() - 1;
	if (desc->num_meshes != scene_meshes) {
		rtk_set_error("rtk_dev_scene_refit: %zu meshes, the scene was made from %zu", (size_t)desc->num_meshes, scene_meshes);
		return RTK_AMD_ERR_BAD_ARG;
	}
	for (size_t mi = 0; mi < desc->num_meshes; mi++) {
		const uint64_t have = ds->mesh_base[mi + 1] - ds->mesh_base[mi];
		if ((uint64_t)desc->meshes[mi].num_triangles != have) {
			rtk_set_error("rtk_dev_scene_refit: mesh %zu has %zu triangles, the scene's has %llu", mi, (size_t)desc->meshes[mi].num_triangles, (unsigned long long)have);
			return RTK_AMD_ERR_BAD_ARG;
		}
	}
	for (size_t mi = 0; mi < desc->num_meshes; mi++) {
		const rtk_mesh *m = &desc->meshes[mi];
		if (m->position_cb) { rtk_set_error("rtk_dev_scene_refit: mesh %zu: position callbacks are not supported by a refit", mi); return RTK_AMD_ERR_UNSUPPORTED; }
		if (m->num_triangles == 0) continue;
		if (m->position.type != RTK_TYPE_DEFAULT && m->position.type != RTK_TYPE_REAL && m->position.type != RTK_TYPE_F32 && m->position.type != RTK_TYPE_F64) {
			rtk_set_error("rtk_dev_scene_refit: mesh %zu: bad position type %d", mi, (int)m->position.type);
			return RTK_AMD_ERR_BAD_ARG;
		}
		if (!m->position.data) { rtk_set_error("rtk_dev_scene_refit: mesh %zu has no positions", mi); return RTK_AMD_ERR_BAD_ARG; }
	}

	const auto t_begin = std::chrono::steady_clock::now();
	std::lock_guard<std::mutex> lock(ds->refit_mutex);
	int before = 0;
	RTK_HIP_CHECK(hipGetDevice(&before), RTK_AMD_ERR_NO_DEVICE);
	if (before != ds->device) RTK_HIP_CHECK(hipSetDevice(ds->device), RTK_AMD_ERR_NO_DEVICE);
	WorkspaceLoan loan;
	const int rc = refit_on_device(ds, desc, (hipStream_t)stream, loan);
	// (a failure may leave work enqueued that reads this call's tables or the workspace: it has to be over first)
	if (rc != RTK_AMD_OK) (void)hipStreamSynchronize((hipStream_t)stream);
	loan.release();
	if (before != ds->device) (void)hipSetDevice(before);
	if (rc == RTK_AMD_OK) ds->refit_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
	return rc;
}

extern "C" double rtk_dev_scene_last_refit_ms(const rtk_dev_scene *ds)
{
	return ds ? ds->refit_ms : 0.0;
}
