// rtk_capsule.hip -- rtk_dev_sweep_capsules / _any: for every query the first time a capsule (a segment with a radius) moving
// along a line touches a device scene, the triangle it touches, the point of the triangle nearest the capsule's axis at that
// time and the point of the axis nearest the triangle, by the rule of rtk_capsule_rule.h. The result is a function of the
// scene's triangle records, the filter and the query alone (DESIGN.md "Capsule sweeps"): the tree only decides which records are
// never looked at.
//
// The walk, the stack and the launch are rtk_sweep_walk.h's; this file is the capsule: the slab routine is rtk_capsule_slab (the
// box grown by g[k] = r + |half_axis[k]| against the path); the side arrays are the points on the triangles and on the axis.
// What the rule forms once per query (g, r2, dd, s and the start's two end points) is formed before the walk.
#include "rtk_sweep_walk.h"
#include "rtk_capsule_rule.h"

namespace {

struct CapsuleSweep {
	typedef rtk_capsule_sweep Sweep;
	typedef rtk_capsule_query Query;
	static constexpr int FLOATS = 12;
	static constexpr const char *NAME = "rtk_dev_sweep_capsules", *NAME_ANY = "rtk_dev_sweep_capsules_any", *NAME_COUNTED = "rtk_dev_sweep_capsules_counted";

	static __device__ __forceinline__ bool prepare(const float *w, Query &Q) { return rtk_capsule_prepare(w, Q); }
	static __device__ __forceinline__ float tmax(const Query &Q) { return Q.S.tmax; }
	static __device__ __forceinline__ bool slab(const Query &Q, const float *lo, const float *hi, float &te) { return rtk_capsule_slab(Q, lo, hi, te); }
	static __device__ __forceinline__ bool touches(const Query &Q, const float *a, const float *b, const float *c, float &time)
	{
		return rtk_capsule_triangle(Q, a, b, c, time) != RTK_CP_NONE;
	}
	// ONE distance walk at the answer's centre. A miss leaves max_t as given, u = v = 0, RTK_PRIM_NONE and the origin
	static __device__ __forceinline__ void record(const Query &Q, const float *w, bool hit, float best_t, uint32_t best_prim,
		const float *a, const float *b, const float *c, sweep_u32x4 &out, float *pt, float *ax)
	{
		out.x = __float_as_uint(w[7]); out.y = 0u; out.z = 0u; out.w = RTK_PRIM_NONE;
		pt[0] = ax[0] = w[0]; pt[1] = ax[1] = w[1]; pt[2] = ax[2] = w[2];
		if (hit) {
			rtk_capsule_contact at;
			rtk_capsule_record(Q, best_t, a, b, c, at);
			pt[0] = at.qt[0]; pt[1] = at.qt[1]; pt[2] = at.qt[2]; ax[0] = at.qa[0]; ax[1] = at.qa[1]; ax[2] = at.qa[2];
			out.x = __float_as_uint(best_t); out.y = __float_as_uint(at.u); out.z = __float_as_uint(at.v); out.w = best_prim;
		}
	}
};

} // namespace

extern "C" uint32_t rtk_amd_capsule_stack_entries(void) { return SWEEP_LDS_STACK; }

int rtk_launch_capsule(const rtk_dev_scene *ds, const rtk_capsule_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_points, float *d_axis_points, uint8_t *d_blocked, bool any_hit, const rtk_dev_filter *filter,
	hipStream_t stream, rtk_trace_counters *counted)
{
	return rtk_launch_sweep_walk<CapsuleSweep>(ds, d_sweeps, num_sweeps, list, d_records, d_points, d_axis_points, d_blocked, any_hit, filter, stream, counted);
}
