// rtk_quant.hip -- DevNode (128 B, exact child boxes) -> DevNodeQ (64 B, 8-bit planes), one thread per node.
// Used after a device build and after a blob upload; see rtk_dev.h for the format and why it exists.
#include "rtk_dev.h"
#include "rtk_node_finish.h"

#include <math.h>

namespace {

// copy_to: also store the exact node there (the device build hands its workspace copy over in the same pass)
__global__ void k_quantize(DevNode *nodes, uint32_t n, DevNodeQ *out, DevNode *copy_to, DevSceneConsts *consts, float bound_hint)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	DevNode nd = nodes[i];
	child_order(nd, nd.order);
	if (copy_to) copy_to[i] = nd;
	else *reinterpret_cast<uint4 *>(nodes[i].order) = make_uint4(nd.order[0], nd.order[1], nd.order[2], nd.order[3]);
	if (i == 0u) {
		// every box of a tree the device builds lies inside the root's (exact unions); an upload passes the bound over all nodes
		const float b = root_bound(nd, bound_hint);
		consts->bound_raw = b;
		consts->bound_abs = fmaxf(b, 1.0f);
	}
	DevNodeQ q;
	const bool misfit = !quantize_node(nd, q);
	out[i] = q;
	// a compressed box that does not contain its exact box would cull real hits: the host then keeps the scene on its exact nodes
	if (misfit) atomicAdd(&consts->qnode_misfits, 1u);
}

// The list form (a refit of some meshes): the nodes list[0 .. *count) only, grid-stride (the count is on the device). What is
// stored for a node is what k_quantize stores for it: both depend on the node's own child boxes and child words alone.
__global__ void __launch_bounds__(256) k_quantize_list(DevNode *nodes, uint32_t n, const uint32_t *list, const uint32_t *count, DevNodeQ *out, DevSceneConsts *consts)
{
	uint32_t total = *count;
	if (total > n) total = n;
	for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
		const uint32_t i = list[e];
		if (i >= n) continue;
		DevNode nd = nodes[i];
		child_order(nd, nd.order);
		*reinterpret_cast<uint4 *>(nodes[i].order) = make_uint4(nd.order[0], nd.order[1], nd.order[2], nd.order[3]);
		if (i == 0u) {
			const float b = root_bound(nd, 0.0f);
			consts->bound_raw = b;
			consts->bound_abs = fmaxf(b, 1.0f);
		}
		DevNodeQ q;
		const bool misfit = !quantize_node(nd, q);
		out[i] = q;
		if (misfit) atomicAdd(&consts->qnode_misfits, 1u);
	}
}

} // namespace

// The scene's constants word block, allocated on first use and cleared on `stream`.
int rtk_scene_consts(rtk_dev_scene *ds, hipStream_t stream)
{
	if (!ds->view.consts) {
		void *c = ds->mem.own(sizeof(DevSceneConsts), 0);
		if (!c) { rtk_set_error("scene constants: %s", hipGetErrorString(hipGetLastError())); return RTK_AMD_ERR_OOM; }
		ds->view.consts = (const DevSceneConsts *)c;
	}
	RTK_HIP_CHECK(hipMemsetAsync(const_cast<DevSceneConsts *>(ds->view.consts), 0, sizeof(DevSceneConsts), stream), RTK_AMD_ERR_HIP);   // (bound_abs 0 = no nodes; kernels read it as max(bound, 1))
	return RTK_AMD_OK;
}

int rtk_quantize_nodes(rtk_dev_scene *ds, hipStream_t stream, const DevNode *src, DevNodeQ *dst, float bound_hint, uint32_t only_first, bool keep_consts, bool readback)
{
	const uint32_t n = ds->view.num_nodes < only_first ? ds->view.num_nodes : only_first;
	void *p = dst;
	if (!keep_consts || !ds->view.consts) { const int rc = rtk_scene_consts(ds, stream); if (rc != RTK_AMD_OK) return rc; }
	DevSceneConsts *consts = const_cast<DevSceneConsts *>(ds->view.consts);
	if (!p) {
		p = ds->mem.own((size_t)(ds->view.num_nodes ? ds->view.num_nodes : 1) * sizeof(DevNodeQ), (size_t)ds->view.num_nodes * sizeof(DevNodeQ));
		if (!p) { rtk_set_error("compressed nodes: %s", hipGetErrorString(hipGetLastError())); return RTK_AMD_ERR_OOM; }
	}
	// src: the nodes still sit in a workspace; ds->view.nodes (allocated, not yet filled) receives them in the same pass
	if (n) hipLaunchKernelGGL(k_quantize, dim3((n + 255u) / 256u), dim3(256), 0, stream, const_cast<DevNode *>(src ? src : ds->view.nodes), n, (DevNodeQ *)p,
		src ? const_cast<DevNode *>(ds->view.nodes) : (DevNode *)nullptr, consts, bound_hint);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	ds->view.qnodes = (const DevNodeQ *)p;
	// the misfit count comes back with the caller's own synchronisation of `stream` (rtk_quantize_finish)
	if (readback) RTK_HIP_CHECK(hipMemcpyAsync(&ds->tree.consts_readback, consts, sizeof(DevSceneConsts), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	return RTK_AMD_OK;
}

int rtk_quantize_node_list(rtk_dev_scene *ds, hipStream_t stream, const uint32_t *list, const uint32_t *d_count)
{
	const uint32_t n = ds->view.num_nodes;
	if (!ds->tree.qnodes_mem || !ds->view.consts) { rtk_set_error("rtk_quantize_node_list: the scene has no compressed nodes"); return RTK_AMD_ERR_BAD_SCENE; }
	const int rc = rtk_scene_consts(ds, stream);
	if (rc != RTK_AMD_OK) return rc;
	DevSceneConsts *consts = const_cast<DevSceneConsts *>(ds->view.consts);
	unsigned blocks = (n + 255u) / 256u;
	if (blocks > 2048u) blocks = 2048u;
	if (n) hipLaunchKernelGGL(k_quantize_list, dim3(blocks), dim3(256), 0, stream, const_cast<DevNode *>(ds->view.nodes), n, list, d_count,
		const_cast<DevNodeQ *>(ds->tree.qnodes_mem), consts);
	RTK_HIP_CHECK(hipGetLastError(), RTK_AMD_ERR_HIP);
	ds->view.qnodes = ds->tree.qnodes_mem;
	RTK_HIP_CHECK(hipMemcpyAsync(&ds->tree.consts_readback, consts, sizeof(DevSceneConsts), hipMemcpyDeviceToHost, stream), RTK_AMD_ERR_HIP);
	return RTK_AMD_OK;
}

// After the stream of rtk_quantize_nodes has been synchronised: a scene with a node that does not fit the 8-bit grid
// (non-finite child extents) is traced with its exact nodes only.
void rtk_quantize_finish(rtk_dev_scene *ds)
{
	ds->tree.bound_abs = ds->tree.consts_readback.bound_abs;
	ds->tree.bound_raw = ds->tree.consts_readback.bound_raw;
	if (ds->view.qnodes) ds->tree.qnodes_mem = ds->view.qnodes;   // (a refit fills the array again and decides anew)
	if (ds->tree.consts_readback.qnode_misfits != 0u) ds->view.qnodes = nullptr;
}
