// rtk_export.hip -- a device-built scene written out in the reference's blob format (host code: the scene is copied home,
// laid out and written by the calling thread).
#include "rtk_dev.h"

#include <string.h>

#include <algorithm>
#include <mutex>
#include <unordered_map>

// =====================================================================================
// export: device BVH -> reference-format blob (writer intent rtk.c:1719-1774)
// =====================================================================================

namespace {

struct ExportPlan {
	std::vector<DevNode> nodes;
	std::vector<DevTri> tris;
	std::vector<uint32_t> vertex_index, slot_mesh, slot_tri;
	// per leaf (in slot order)
	struct Leaf { uint32_t first, count; uint64_t offset; uint64_t group_byte; uint32_t num_meshes; std::vector<uint8_t> vix; };
	std::vector<Leaf> leaves;
	std::unordered_map<uint32_t, uint32_t> leaf_of_slot;
	std::vector<rtk_vertex> vertices;
	uint64_t node_off = 128, leaf_off = 0, vert_off = 0, total = 0;
};

size_t align_up(size_t v, size_t a) { return (v + a - 1) & ~(a - 1); }

bool download(const rtk_dev_scene *ds, ExportPlan &ep)
{
	if (rtk_scene_side_arrays(ds, nullptr) != RTK_AMD_OK) return false;
	const DevSceneView &v = ds->view;
	ep.nodes.resize(v.num_nodes);
	ep.tris.resize(v.num_tris);
	ep.vertex_index.resize(3 * (size_t)v.num_tris);
	ep.slot_mesh.resize(v.num_tris);
	ep.slot_tri.resize(v.num_tris);
	bool ok = hipMemcpy(ep.nodes.data(), v.nodes, ep.nodes.size() * sizeof(DevNode), hipMemcpyDeviceToHost) == hipSuccess;
	if (v.num_tris) {
		ok = ok && hipMemcpy(ep.tris.data(), v.tris, ep.tris.size() * sizeof(DevTri), hipMemcpyDeviceToHost) == hipSuccess;
		ok = ok && hipMemcpy(ep.vertex_index.data(), v.vertex_index, ep.vertex_index.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
		ok = ok && hipMemcpy(ep.slot_mesh.data(), v.slot_mesh, ep.slot_mesh.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
		ok = ok && hipMemcpy(ep.slot_tri.data(), v.slot_tri, ep.slot_tri.size() * 4, hipMemcpyDeviceToHost) == hipSuccess;
	}
	if (!ok) rtk_set_error("export: device to host copy failed: %s", hipGetErrorString(hipGetLastError()));
	return ok;
}

// Lay out leaves and vertex groups. Leaves are visited in slot order (= Morton order), so
// consecutive leaves are neighbours in space and share vertices of indexed meshes; a
// vertex group (<= 256 vertices, u8 indices, rtk.c:83, 1186) is closed when the next leaf
// would not fit.
bool plan(ExportPlan &ep)
{
	std::vector<uint32_t> firsts;
	for (const DevNode &n : ep.nodes)
		for (int k = 0; k < 4; k++)
			if (n.child[k] != RTK_REF_NONE && (n.child[k] & RTK_REF_LEAF)) firsts.push_back(n.child[k] & 0x7fffffffu);
	std::sort(firsts.begin(), firsts.end());
	firsts.erase(std::unique(firsts.begin(), firsts.end()), firsts.end());
	ep.leaves.resize(firsts.size());
	std::unordered_map<uint64_t, uint32_t> group;   // (mesh<<32 | vertex index) -> index in the open group
	size_t group_start = 0;                          // in vertices
	uint64_t leaf_bytes = 64;                        // null leaf first (rtk.c:1763-1765)
	for (size_t li = 0; li < firsts.size(); li++) {
		ExportPlan::Leaf &lf = ep.leaves[li];
		lf.first = firsts[li];
		if (lf.first >= ep.tris.size()) { rtk_set_error("export: leaf reference out of range"); return false; }
		lf.count = ep.tris[lf.first].spare;
		if (lf.count == 0 || lf.count > 63 || (size_t)lf.first + lf.count > ep.tris.size()) { rtk_set_error("export: leaf of %u triangles cannot be written (1..63)", lf.count); return false; }
		ep.leaf_of_slot[lf.first] = (uint32_t)li;
		// distinct vertices this leaf would add
		std::vector<uint64_t> keys(3 * (size_t)lf.count);
		for (uint32_t i = 0; i < lf.count; i++)
			for (int c = 0; c < 3; c++)
				keys[3 * i + c] = ((uint64_t)ep.slot_mesh[lf.first + i] << 32) | ep.vertex_index[3 * (size_t)(lf.first + i) + c];
		size_t fresh = 0;
		{
			std::vector<uint64_t> uniq(keys);
			std::sort(uniq.begin(), uniq.end());
			uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
			for (uint64_t k : uniq) if (!group.count(k)) fresh++;
		}
		if (group.size() + fresh > 256) {
			group.clear();
			group_start = align_up(ep.vertices.size(), 4);    // 64-byte aligned groups (rtk.c:193)
			ep.vertices.resize(group_start);
		}
		lf.group_byte = (uint64_t)group_start * 16u;
		lf.vix.resize(3 * (size_t)lf.count);
		std::vector<uint32_t> meshes;
		for (uint32_t i = 0; i < lf.count; i++) {
			const DevTri &t = ep.tris[lf.first + i];
			const float *pv[3] = { t.v0, t.v1, t.v2 };
			for (int c = 0; c < 3; c++) {
				const uint64_t k = keys[3 * i + c];
				auto it = group.find(k);
				uint32_t idx;
				if (it == group.end()) {
					idx = (uint32_t)group.size();
					group[k] = idx;
					rtk_vertex v;
					v.position.x = pv[c][0]; v.position.y = pv[c][1]; v.position.z = pv[c][2];
					v.index = (uint32_t)k;
					ep.vertices.push_back(v);
				} else idx = it->second;
				lf.vix[3 * i + c] = (uint8_t)idx;
			}
			const uint32_t mesh = ep.slot_mesh[lf.first + i];
			if (std::find(meshes.begin(), meshes.end(), mesh) == meshes.end()) meshes.push_back(mesh);
		}
		lf.num_meshes = (uint32_t)meshes.size();
		lf.offset = leaf_bytes;
		leaf_bytes += align_up(8 + 8 * (size_t)((lf.count + 3u) & ~3u) + 4 * meshes.size(), 64);
	}
	ep.leaf_off = align_up(ep.node_off + ep.nodes.size() * 128, 128);
	ep.vert_off = align_up(ep.leaf_off + leaf_bytes, 128);
	ep.total = align_up(ep.vert_off + align_up(ep.vertices.size(), 4) * 16, 128);
	return true;
}

void write_blob(const ExportPlan &ep, char *blob)
{
	memset(blob, 0, ep.total);
	rtk_scene *s = (rtk_scene *)blob;
	static const char magic[8] = { 0, 'R', 'T', 'K', '\r', '\n', 0x1a, '\n' };
	memcpy(s->magic, magic, 8);
	s->endian = 0xaabb; s->sizeof_real = 4; s->pad_0 = 0; s->version = 1; s->pad_1 = 0;
	s->size_in_bytes = ep.total; s->node_offset = ep.node_off; s->leaf_offset = ep.leaf_off; s->vertex_offset = ep.vert_off;
	for (size_t i = 0; i < ep.nodes.size(); i++) {
		const DevNode &n = ep.nodes[i];
		char *dst = blob + ep.node_off + i * 128;
		memcpy(dst, n.bx, 96);
		uint64_t ptr[4];
		for (int k = 0; k < 4; k++) {
			const uint32_t r = n.child[k];
			if (r == RTK_REF_NONE) ptr[k] = ep.leaf_off | 1u;                               // null leaf (rtk.c:1619, tagged: B19)
			else if (r & RTK_REF_LEAF) ptr[k] = (ep.leaf_off + ep.leaves[ep.leaf_of_slot.at(r & 0x7fffffffu)].offset) | 1u;
			else ptr[k] = ep.node_off + (uint64_t)r * 128u;
		}
		memcpy(dst + 96, ptr, 32);
	}
	for (const ExportPlan::Leaf &lf : ep.leaves) {
		char *dst = blob + ep.leaf_off + lf.offset;
		const uint64_t info = (uint64_t)lf.count | (ep.vert_off + lf.group_byte);
		memcpy(dst, &info, 8);
		const size_t n4 = (lf.count + 3u) & ~3u;
		uint32_t *table = (uint32_t *)(dst + 8 + 8 * n4);
		uint32_t nm = 0;
		for (uint32_t i = 0; i < lf.count; i++) {
			uint8_t *rec = (uint8_t *)dst + 8 + 8 * (size_t)i;
			rec[0] = lf.vix[3 * i]; rec[1] = lf.vix[3 * i + 1]; rec[2] = lf.vix[3 * i + 2];
			const uint32_t mesh = ep.slot_mesh[lf.first + i];
			uint32_t k = 0;
			for (; k < nm; k++) if (table[k] == mesh) break;
			if (k == nm) table[nm++] = mesh;
			rec[3] = (uint8_t)k;
			memcpy(rec + 4, &ep.slot_tri[lf.first + i], 4);
		}
	}
	if (!ep.vertices.empty()) memcpy(blob + ep.vert_off, ep.vertices.data(), ep.vertices.size() * 16);
}

// one export plan is cached per scene between export_size and export
std::mutex g_plans_mutex;
std::unordered_map<const rtk_dev_scene *, ExportPlan *> g_plans;

ExportPlan *get_plan(const rtk_dev_scene *ds)
{
	std::lock_guard<std::mutex> lock(g_plans_mutex);
	auto it = g_plans.find(ds);
	if (it != g_plans.end()) return it->second;
	ExportPlan *ep = new ExportPlan();
	if (!download(ds, *ep) || !plan(*ep)) { delete ep; return nullptr; }
	g_plans[ds] = ep;
	return ep;
}

void drop_plan(const rtk_dev_scene *ds)
{
	std::lock_guard<std::mutex> lock(g_plans_mutex);
	auto it = g_plans.find(ds);
	if (it != g_plans.end()) { delete it->second; g_plans.erase(it); }
}

} // namespace

void rtk_export_forget(const rtk_dev_scene *ds) { drop_plan(ds); }

extern "C" size_t rtk_dev_scene_export_size(const rtk_dev_scene *ds)
{
	if (!ds) { rtk_set_error("rtk_dev_scene_export_size: NULL scene"); return 0; }
	ExportPlan *ep = get_plan(ds);
	return ep ? (size_t)ep->total : 0;
}

extern "C" rtk_scene *rtk_dev_scene_export(const rtk_dev_scene *ds, void *buffer, size_t size)
{
	if (!ds || !buffer) { rtk_set_error("rtk_dev_scene_export: NULL argument"); return nullptr; }
	ExportPlan *ep = get_plan(ds);
	if (!ep) return nullptr;
	if (size < ep->total) { rtk_set_error("rtk_dev_scene_export: buffer too small (%zu < %llu)", size, (unsigned long long)ep->total); return nullptr; }
	write_blob(*ep, (char *)buffer);
	drop_plan(ds);
	return (rtk_scene *)buffer;
}
