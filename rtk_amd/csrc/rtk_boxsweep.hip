// rtk_boxsweep.hip -- rtk_dev_sweep_boxes / _any: for every query the first time an axis-aligned box moving along a line touches
// a device scene, the triangle it touches, the centre at that time and the contact normal, by the rule of rtk_boxsweep_rule.h. The
// result is a function of the scene's triangle records, the filter and the query alone (DESIGN.md "Box sweeps"): the tree only
// decides which records are never looked at.
//
// The walk, the stack and the launch are rtk_sweep_walk.h's; this file is the box: the slab routine is rtk_boxsweep_slab (the box
// grown by the half extents against the path of the centre); the rule's triangle routine computes the edges and the normal once
// per record and the thirteen axes from them; the side arrays are the centres and the normals. The normal is the answer's alone:
// the winning axis is found again by ONE more evaluation of the answer's triangle at the end.
#include "rtk_sweep_walk.h"
#include "rtk_boxsweep_rule.h"

namespace {

struct BoxSweep {
	typedef rtk_box_sweep Sweep;
	typedef rtk_boxsweep_query Query;
	static constexpr int FLOATS = 11;
	static constexpr const char *NAME = "rtk_dev_sweep_boxes", *NAME_ANY = "rtk_dev_sweep_boxes_any", *NAME_COUNTED = "rtk_dev_sweep_boxes_counted";

	static __device__ __forceinline__ bool prepare(const float *w, Query &Q) { return rtk_boxsweep_prepare(w, Q); }
	static __device__ __forceinline__ float tmax(const Query &Q) { return Q.tmax; }
	static __device__ __forceinline__ bool slab(const Query &Q, const float *lo, const float *hi, float &te)
	{
		float tx;
		int face;
		return rtk_boxsweep_slab(Q, lo, hi, te, tx, face);
	}
	static __device__ __forceinline__ bool touches(const Query &Q, const float *a, const float *b, const float *c, float &time)
	{
		return rtk_boxsweep_triangle(Q, a, b, c, time) != RTK_BS_NONE;
	}
	// ONE evaluation at the answer's centre, and the answer's triangle once more for the axis that gave its time. A miss leaves
	// max_t as given, u = v = 0, RTK_PRIM_NONE, the origin and a normal of zeros
	static __device__ __forceinline__ void record(const Query &Q, const float *w, bool hit, float best_t, uint32_t best_prim,
		const float *a, const float *b, const float *c, sweep_u32x4 &out, float *ct, float *nm)
	{
		out.x = __float_as_uint(w[7]); out.y = 0u; out.z = 0u; out.w = RTK_PRIM_NONE;
		ct[0] = w[0]; ct[1] = w[1]; ct[2] = w[2]; nm[0] = nm[1] = nm[2] = 0.0f;
		if (hit) {
			float u, v, q[3], time;
			int region;
			rtk_boxsweep_centre(Q, best_t, ct);
			(void)rtk_closest_triangle(ct, a, b, c, q, u, v, region);
			rtk_boxsweep_normal(Q, a, b, c, rtk_boxsweep_triangle(Q, a, b, c, time), nm);
			out.x = __float_as_uint(best_t); out.y = __float_as_uint(u); out.z = __float_as_uint(v); out.w = best_prim;
		}
	}
};

} // namespace

extern "C" uint32_t rtk_amd_boxsweep_stack_entries(void) { return SWEEP_LDS_STACK; }

int rtk_launch_boxsweep(const rtk_dev_scene *ds, const rtk_box_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_centres, float *d_normals, uint8_t *d_blocked, bool any_hit, const rtk_dev_filter *filter,
	hipStream_t stream, rtk_trace_counters *counted)
{
	return rtk_launch_sweep_walk<BoxSweep>(ds, d_sweeps, num_sweeps, list, d_records, d_centres, d_normals, d_blocked, any_hit, filter, stream, counted);
}
