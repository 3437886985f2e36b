// rtk_quality.hip -- how good is the tree a device scene has NOW (rtk_dev_scene_quality): the surface-area-heuristic
// cost of its exact nodes, measured on the device. What a host that refits every frame compares against the cost right
// after the build to decide when a rebuild pays.
//
// For a ray that enters the root's box, the chance of entering a child box is about area(child) / area(root). So
//   node_visits    = 1 + sum of the areas of all inner child boxes / root_area
//   triangle_tests = sum over leaf children of area * triangles in the leaf / root_area
//   sah_cost       = cost_node * node_visits + cost_tri * triangle_tests      (the builder's two constants, rtk_sah_costs)
// The sums are over the exact child boxes of the 128-byte nodes (the compressed ones are their conservative images) and the
// leaf sizes in the first record of every leaf (DevTri.spare). Nothing in the scene is written.
//   k_quality_partials   one pass over the nodes, four lanes per node as k_refit_level has them (one per child slot; a wave
//                        reads 16 whole lines). A FIXED grid strides over the nodes; every lane adds its terms in double in
//                        the order of its trips, the lanes of a wave are added by a butterfly, the waves of a workgroup
//                        through LDS in wave order, and thread 0 stores the workgroup's record.
//   k_quality_finish     one workgroup: the records added in index order, the root's area from node 0.
// DETERMINISM: the same scene bits give the same result bits, on every call. No floating-point atomic; who adds what to
// what in which order is decided by the launch shape alone, which does not depend on the scene (QUALITY_BLOCKS records
// whatever its size). The second launch sees the first one's records through the kernel boundary (as a refit's heights
// see each other, rtk_refit.hip): no fence, no counter handed between workgroups.
#include "rtk_dev.h"

#include <math.h>
#include <string.h>


namespace {

#define QUALITY_THREADS 512                    // four lanes per node: 128 nodes per workgroup and trip
#define QUALITY_WAVES (QUALITY_THREADS / 64)
#define QUALITY_BLOCKS 1024u                   // the grid, and the number of partial records, for every scene
#define QUALITY_FINISH_THREADS 256

// what one workgroup found (64 B), and what the second launch makes of all of them
struct QualityPartial {
	double area[3];                            // inner child boxes, leaf child boxes, leaf child boxes * triangles in the leaf
	unsigned long long count[3];               // inner children, leaf children, boxes whose area is not finite
	unsigned long long pad[2];
};
static_assert(sizeof(QualityPartial) == 64, "QualityPartial");
struct QualityResult {
	QualityPartial sum;
	double root_area;
	double pad[7];
};
static_assert(sizeof(QualityResult) == 128, "QualityResult");

// 2 * (dx*dy + dy*dz + dz*dx) in double from the float planes, in exactly this order (the tests restate it)
__device__ __forceinline__ double box_area(float x0, float x1, float y0, float y1, float z0, float z1)
{
	const double dx = (double)x1 - (double)x0, dy = (double)y1 - (double)y0, dz = (double)z1 - (double)z0;
	return 2.0 * (dx * dy + dy * dz + dz * dx);
}

__global__ void __launch_bounds__(QUALITY_THREADS) k_quality_partials(const DevNode *nodes, uint32_t num_nodes, const DevTri *tris, uint32_t num_tris,
	QualityPartial *partials)
{
	double a_inner = 0.0, a_leaf = 0.0, a_leaf_tris = 0.0;
	uint32_t n_inner = 0, n_leaf = 0, n_bad = 0;               // (a lane meets num_nodes / (QUALITY_BLOCKS * 128) + 1 slots at most)
	const uint32_t k = threadIdx.x & 3u;
	const unsigned long long step = (unsigned long long)gridDim.x * (QUALITY_THREADS / 4);
	for (unsigned long long i = (unsigned long long)blockIdx.x * (QUALITY_THREADS / 4) + (threadIdx.x >> 2); i < num_nodes; i += step) {
		const DevNode *nd = nodes + i;
		const uint32_t ref = nd->child[k];
		const float x0 = nd->bx[0][k], x1 = nd->bx[1][k], y0 = nd->by[0][k], y1 = nd->by[1][k], z0 = nd->bz[0][k], z1 = nd->bz[1][k];
		if (ref == RTK_REF_NONE) continue;                       // an empty slot, whatever its planes hold
		const double area = box_area(x0, x1, y0, y1, z0, z1);
		if (ref & RTK_REF_LEAF) {
			const uint32_t first = ref & 0x7fffffffu;
			const uint32_t cnt = first < num_tris ? tris[first].spare : 0u;
			n_leaf++;
			if (isfinite(area)) { a_leaf += area; a_leaf_tris += area * (double)cnt; } else n_bad++;
		} else {
			n_inner++;
			if (isfinite(area)) a_inner += area; else n_bad++;
		}
	}
	// the wave: a butterfly, after which every lane holds the same sum (a + b == b + a)
	for (int o = 32; o > 0; o >>= 1) {
		a_inner += __shfl_xor(a_inner, o);
		a_leaf += __shfl_xor(a_leaf, o);
		a_leaf_tris += __shfl_xor(a_leaf_tris, o);
		n_inner += __shfl_xor(n_inner, o);
		n_leaf += __shfl_xor(n_leaf, o);
		n_bad += __shfl_xor(n_bad, o);
	}
	// the workgroup: wave 0 first, wave 7 last
	__shared__ double s_area[QUALITY_WAVES][3];
	__shared__ uint32_t s_count[QUALITY_WAVES][3];
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	if (lane == 0u) {
		s_area[wave][0] = a_inner; s_area[wave][1] = a_leaf; s_area[wave][2] = a_leaf_tris;
		s_count[wave][0] = n_inner; s_count[wave][1] = n_leaf; s_count[wave][2] = n_bad;
	}
	__syncthreads();
	if (threadIdx.x == 0u) {
		QualityPartial p = {};
		for (uint32_t w = 0; w < QUALITY_WAVES; w++) {
			for (int f = 0; f < 3; f++) { p.area[f] += s_area[w][f]; p.count[f] += s_count[w][f]; }
		}
		partials[blockIdx.x] = p;
	}
}

// One workgroup. The records go to LDS side by side; then one lane per sum walks its column from record 0 to the last (the
// three areas in wave 0, the three counts in wave 1, the root in wave 2: no wave runs two of them one after the other).
__global__ void __launch_bounds__(QUALITY_FINISH_THREADS) k_quality_finish(const QualityPartial *partials, const DevNode *nodes, uint32_t num_nodes, QualityResult *result)
{
	__shared__ double s_area[3][QUALITY_BLOCKS];
	__shared__ unsigned long long s_count[3][QUALITY_BLOCKS];
	for (uint32_t i = threadIdx.x; i < QUALITY_BLOCKS; i += QUALITY_FINISH_THREADS) {
		const QualityPartial p = partials[i];
		for (int f = 0; f < 3; f++) { s_area[f][i] = p.area[f]; s_count[f][i] = p.count[f]; }
	}
	__syncthreads();
	if (threadIdx.x < 3u) {
		double s = 0.0;
		for (uint32_t i = 0; i < QUALITY_BLOCKS; i++) s += s_area[threadIdx.x][i];
		result->sum.area[threadIdx.x] = s;
	} else if (threadIdx.x >= 64u && threadIdx.x < 67u) {
		unsigned long long s = 0;
		for (uint32_t i = 0; i < QUALITY_BLOCKS; i++) s += s_count[threadIdx.x - 64u][i];
		result->sum.count[threadIdx.x - 64u] = s;
	} else if (threadIdx.x == 128u) {
		// the root's box: the union of node 0's non-empty child boxes, as a refit forms a union (it starts from its first
		// member and grows by fminf / fmaxf, which skip a NaN)
		double area = 0.0;
		if (num_nodes) {
			float mn[3] = { 0.0f, 0.0f, 0.0f }, mx[3] = { 0.0f, 0.0f, 0.0f };
			bool first_member = true;
			for (int q = 0; q < 4; q++) {
				if (nodes[0].child[q] == RTK_REF_NONE) continue;
				const float lo[3] = { nodes[0].bx[0][q], nodes[0].by[0][q], nodes[0].bz[0][q] };
				const float hi[3] = { nodes[0].bx[1][q], nodes[0].by[1][q], nodes[0].bz[1][q] };
				for (int ax = 0; ax < 3; ax++) {
					mn[ax] = first_member ? lo[ax] : fminf(mn[ax], lo[ax]);
					mx[ax] = first_member ? hi[ax] : fmaxf(mx[ax], hi[ax]);
				}
				first_member = false;
			}
			if (!first_member) area = box_area(mn[0], mx[0], mn[1], mx[1], mn[2], mx[2]);
		}
		result->root_area = area;
	}
}

// partial records and the result slot: made by the scene's first measurement and kept (no later call allocates)
int make_buffers(rtk_dev_scene *ds)
{
	if (ds->quality.d_mem) return RTK_AMD_OK;
	const size_t bytes = QUALITY_BLOCKS * sizeof(QualityPartial) + sizeof(QualityResult);
	ds->quality.d_mem = ds->mem.own(bytes, bytes);
	if (!ds->quality.d_mem) { (void)hipGetLastError(); rtk_set_error("rtk_dev_scene_quality: out of device memory"); return RTK_AMD_ERR_OOM; }
	return RTK_AMD_OK;
}

// the scene's device is current
int measure_on_device(rtk_dev_scene *ds, hipStream_t stream, QualityResult *res)
{
	const int rc = make_buffers(ds);
	if (rc != RTK_AMD_OK) return rc;
	const DevSceneView &v = ds->view;
	QualityPartial *partials = (QualityPartial *)ds->quality.d_mem;
	QualityResult *d_result = (QualityResult *)(partials + QUALITY_BLOCKS);
	hipLaunchKernelGGL(k_quality_partials, dim3(QUALITY_BLOCKS), dim3(QUALITY_THREADS), 0, stream, v.nodes, v.num_nodes, v.tris, v.num_tris, partials);
	hipLaunchKernelGGL(k_quality_finish, dim3(1), dim3(QUALITY_FINISH_THREADS), 0, stream, partials, v.nodes, v.num_nodes, d_result);
	RTK_PASS_CHECK("rtk_dev_scene_quality", hipGetLastError());
	RTK_PASS_CHECK("rtk_dev_scene_quality", hipMemcpyAsync(res, d_result, sizeof(QualityResult), hipMemcpyDeviceToHost, stream));
	RTK_PASS_CHECK("rtk_dev_scene_quality", hipStreamSynchronize(stream));
	return RTK_AMD_OK;
}

} // namespace

extern "C" int rtk_dev_scene_quality(const rtk_dev_scene *scene, rtk_dev_scene_quality_info *out, void *stream)
{
	// ---- everything that can be refused is refused here, before HIP is touched
	if (!scene || !out) { rtk_set_error("rtk_dev_scene_quality: NULL argument"); return RTK_AMD_ERR_BAD_ARG; }
	if (out->struct_size < sizeof(rtk_dev_scene_quality_info)) {
		rtk_set_error("rtk_dev_scene_quality: struct_size %u, rtk_dev_scene_quality_info has %zu bytes", out->struct_size, sizeof(rtk_dev_scene_quality_info));
		return RTK_AMD_ERR_BAD_ARG;
	}
	rtk_dev_scene *ds = const_cast<rtk_dev_scene *>(scene);      // (the buffers and the remembered cost are the scene's; no bit a trace reads changes)
	ScenePass pass(ds, stream);                                  // never beside a refit; one measurement of a scene at a time (they share the records)
	const uint32_t struct_size = out->struct_size;
	memset(out, 0, sizeof(*out));
	out->struct_size = struct_size;
	QualityResult res = {};
	if (ds->view.num_tris != 0u && ds->view.num_nodes != 0u) {
		if (!pass.on_device()) return RTK_AMD_ERR_NO_DEVICE;
		const int rc = pass.end(measure_on_device(ds, pass.stream, &res));
		if (rc != RTK_AMD_OK) return rc;
	}
	out->nonfinite_boxes = res.sum.count[2] > 0xffffffffull ? 0xffffffffu : (uint32_t)res.sum.count[2];
	out->inner_children = res.sum.count[0];
	out->leaf_children = res.sum.count[1];
	out->root_area = res.root_area;
	out->inner_area = res.sum.area[0];
	out->leaf_area = res.sum.area[1];
	out->leaf_area_triangles = res.sum.area[2];
	if (isfinite(res.root_area) && res.root_area != 0.0) {
		float cost_node = 0.0f, cost_tri = 0.0f;
		rtk_sah_costs(&cost_node, &cost_tri);
		out->node_visits = 1.0 + out->inner_area / res.root_area;
		out->triangle_tests = out->leaf_area_triangles / res.root_area;
		out->sah_cost = (double)cost_node * out->node_visits + (double)cost_tri * out->triangle_tests;
	}
	// the cost the scene had before anything moved: the first measurement, if no refit came before it
	if (!ds->quality.baseline_known && !ds->quality.refitted) {
		ds->quality.baseline_known = true;
		ds->quality.sah_cost_at_build = out->sah_cost;
	}
	out->sah_cost_at_build = ds->quality.baseline_known ? ds->quality.sah_cost_at_build : 0.0;
	out->measure_ms = pass.ms();
	return RTK_AMD_OK;
}
