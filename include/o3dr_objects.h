/* o3dr_objects.h - object operators on a cloud (libo3dr.so; o3dr.h holds the context, the point layout, the error codes
 * and the memory kinds this header builds on). */
#ifndef O3DR_OBJECTS_H
#define O3DR_OBJECTS_H
#include "o3dr.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- Euclidean clustering: which points belong to the same object.  The family is pcl::EuclideanClusterExtraction: two
 * points closer than a tolerance are linked, and an object is a class of the links' transitive closure.  The reference has
 * no such tool; the contract is this library's own.  The partition does not depend on the order
 * in which links are found, and everything derived from it is an integer, a copy, a min / max or an exact integer sum:
 * results are bit-identical across calls, memory kinds and whatever search structure finds the links.
 *
 * Input: n points, n < 2^31, every coordinate finite; tolerance finite and > 0 with r2 = (float)(tolerance * tolerance)
 * (the product in fp64) finite and > 0; 1 <= min_size <= max_size; every side of the cloud's bounding box, (double)max -
 * (double)min per axis, < 32768 metres (step 5 needs it).
 *   1. Link: points i != j are linked iff d2 = ((0 + dx*dx) + dy*dy) + dz*dz <= r2, in fp32 without FMA, d = p_i - p_j:
 *      the d2 of o3dr_nearest_neighbors.  It is symmetric (fp32 subtraction is antisymmetric); duplicate points are linked.
 *   2. Components: a component is a class of the transitive closure of the links.  raw[i] is the lowest point index of
 *      i's component and size[i] its point count, both before any rejection (as the disparity filter's labels / sizes).
 *   3. Clusters: a component is a cluster iff min_size <= size <= max_size.  Clusters are numbered 0 .. K-1 in ascending
 *      raw; label[i] is the cluster's number, or -1 for a point of a rejected component.
 *   4. indices (PCL's PointIndices): the points of the clusters, cluster by cluster in number order, each cluster's points
 *      in ascending index; n_clustered_points entries.
 *   5. One o3dr_cluster per cluster, in number order: first = raw; size; begin = where the cluster starts in indices (the
 *      exclusive sum of the sizes in number order, filled whether or not indices is asked for); reserved = 0; lo / hi = the
 *      min / max of the members' coordinates, each taken as c + 0.0f (-0.0f counts as 0.0f: min / max are order-free);
 *      centroid, exact from integer sums: per axis q_i = (int64)floor(((double)c_i - (double)lo) * 65536.0 + 0.5), S = the
 *      int64 sum of the q_i (q_i <= 2^31, so it cannot overflow), centroid = (double)lo + ((double)S / 65536.0) /
 *      (double)size, every operation in fp64 as written, no FMA.  The sums are integers: any order gives the same bits.
 *   6. o3dr_cluster_result: n_components; n_clusters + n_too_small + n_too_large = n_components; n_clustered_points +
 *      n_rejected_points = n; largest = the size of the largest component; n_pairs = the unordered pairs i < j that are
 *      linked (it checks the neighbour search itself, not only its closure).
 * clusters holds clusters_capacity records and *n_clusters is always set to K.  With clusters set and K > clusters_capacity
 * the call returns O3DR_ERR_CAPACITY with *n_clusters set and writes nothing else (o3dr_mesh_surface's rule); clusters NULL
 * with capacity 0 gives the counts and the point outputs only.
 * Errors, O3DR_ERR_INVALID_ARG, in this order: a bad parameter, in the struct's order (tolerance or r2 not finite or not
 * > 0; min_size < 1; max_size < min_size); the cloud (a non-finite coordinate; a box side >= 32768 m).  All are found
 * before any grid work; a bad parameter launches nothing.  On an error the host outputs and the result are zeroed.
 * n == 0 is allowed: no component.  The call synchronises and reuses the operators' scratch and the sort workspace:
 * cloud_big is left alone. */
typedef struct o3dr_cluster_params {
    double tolerance;   /* > 0, finite; no usable default (0 is rejected): a few voxel sizes of the map */
    int32_t min_size;   /* 1: pcl::EuclideanClusterExtraction min_pts_per_cluster_ */
    int32_t max_size;   /* 2^31 - 1: max_pts_per_cluster_ */
} o3dr_cluster_params;
typedef struct o3dr_cluster {
    int32_t first;      /* the cluster's lowest point index (raw) */
    int32_t size;
    int32_t begin;      /* the cluster's first entry in indices */
    int32_t reserved;   /* 0 */
    float lo[3], hi[3];
    double centroid[3];
} o3dr_cluster;         /* 64 bytes */
typedef struct o3dr_cluster_outputs {
    int32_t* label;     /* n: the cluster's number, -1: rejected */
    int32_t* raw;       /* n: the lowest index of the point's component */
    int32_t* size;      /* n: the component's point count */
    int32_t* indices;   /* n (n_clustered_points written) */
} o3dr_cluster_outputs;
typedef struct o3dr_cluster_result {
    int64_t n_components, n_clusters, n_too_small, n_too_large;
    int64_t n_clustered_points, n_rejected_points;
    int64_t largest;
    int64_t n_pairs;
} o3dr_cluster_result;
void o3dr_cluster_default_params(o3dr_cluster_params* p);
int  o3dr_cluster_euclidean(o3dr_ctx* ctx, const o3dr_point* cloud, int64_t n, const o3dr_cluster_params* p,
                            const o3dr_cluster_outputs* out, o3dr_cluster* clusters, int64_t clusters_capacity,
                            int64_t* n_clusters, o3dr_cluster_result* res, int32_t mem);

#ifdef __cplusplus
}
#endif
#endif
