// rtk_sweep.hip -- rtk_dev_sweep_spheres / _any: for every query the first time a ball moving along a line touches a device
// scene, the triangle it touches, the contact point and the centre at that time, by the rule of rtk_sweep_rule.h. The result is
// a function of the scene's triangle records, the filter and the query alone (DESIGN.md "Sphere sweeps"): the tree only decides
// which records are never looked at.
//
// The walk, the stack and the launch are rtk_sweep_walk.h's; this file is the ball: the slab routine is rtk_sweep_slab (the box
// grown by the radius against the path), the side arrays are the contact points and the centres.
#include "rtk_sweep_walk.h"
#include "rtk_sweep_rule.h"

namespace {

struct SphereSweep {
	typedef rtk_sphere_sweep Sweep;
	typedef rtk_sweep_query Query;
	static constexpr int FLOATS = 9;
	static constexpr const char *NAME = "rtk_dev_sweep_spheres", *NAME_ANY = "rtk_dev_sweep_spheres_any", *NAME_COUNTED = "rtk_dev_sweep_spheres_counted";

	static __device__ __forceinline__ bool prepare(const float *w, Query &Q) { return rtk_sweep_prepare(w, Q); }
	static __device__ __forceinline__ float tmax(const Query &Q) { return Q.tmax; }
	static __device__ __forceinline__ bool slab(const Query &Q, const float *lo, const float *hi, float &te) { return rtk_sweep_slab(Q, lo, hi, te); }
	static __device__ __forceinline__ bool touches(const Query &Q, const float *a, const float *b, const float *c, float &time)
	{
		return rtk_sweep_triangle(Q, a, b, c, time) != RTK_SW_NONE;
	}
	// ONE evaluation at the answer's centre. A miss leaves max_t as given, u = v = 0, RTK_PRIM_NONE and the origin
	static __device__ __forceinline__ void record(const Query &Q, const float *w, bool hit, float best_t, uint32_t best_prim,
		const float *a, const float *b, const float *c, sweep_u32x4 &out, float *pt, float *ct)
	{
		out.x = __float_as_uint(w[7]); out.y = 0u; out.z = 0u; out.w = RTK_PRIM_NONE;
		pt[0] = ct[0] = w[0]; pt[1] = ct[1] = w[1]; pt[2] = ct[2] = w[2];
		if (hit) {
			float u, v;
			int region;
			rtk_sweep_centre(Q, best_t, ct);
			(void)rtk_closest_triangle(ct, a, b, c, pt, u, v, region);
			out.x = __float_as_uint(best_t); out.y = __float_as_uint(u); out.z = __float_as_uint(v); out.w = best_prim;
		}
	}
};

} // namespace

extern "C" uint32_t rtk_amd_sweep_stack_entries(void) { return SWEEP_LDS_STACK; }

int rtk_launch_sweep(const rtk_dev_scene *ds, const rtk_sphere_sweep *d_sweeps, size_t num_sweeps, const rtk_ray_list *list,
	rtk_hit_record *d_records, float *d_points, float *d_centres, uint8_t *d_blocked, bool any_hit, const rtk_dev_filter *filter,
	hipStream_t stream, rtk_trace_counters *counted)
{
	return rtk_launch_sweep_walk<SphereSweep>(ds, d_sweeps, num_sweeps, list, d_records, d_points, d_centres, d_blocked, any_hit, filter, stream, counted);
}
