// o3dr_host.h — C++ host mirror of the reference's `Pose` class for the reconstruction hot path.
//
// Same member-function names, argument meaning and error behaviour as pose.h:198,199,216,231 of the
// reference; the bodies call libo3dr (include/o3dr.h) instead of OpenCV/PCL.  Everything outside the
// hot path that the CLI needs to run end to end (flag parsing, calibration/pose/time CSV readers,
// timestamp binding, generateTmat, the variance gate, PNG/PLY I/O) is restated here in plain C++:
// it is control plane, one call per frame or per run, and stays on the host.  The ICP trajectory correction,
// visualisation and --segment_cloud in a reconstruction run are not part of this build; by default the CLI runs with the
// recorded MAVLink poses (the reference's --only_MAVLink mode, pose_functions.cpp:232-236), with --feature_poses every
// frame's pose comes from o3dr_pose_chain (the reference's default mode, pose.cpp:213-235).  The --align_point_cloud tool (ICP on two PLYs) runs on o3dr_icp_align, the
// --smooth_surface tool (MLS on one PLY) on o3dr_mls_smooth, the --segment_cloud_only tool (RANSAC planes per XY tile on
// one PLY) on o3dr_segment_plane, the --mesh_surface tool (a height-field triangulation of one PLY) on o3dr_mesh_surface,
// the --orthophoto tool (orthophoto, elevation raster and shaded relief of one PLY) on o3dr_rasterize_map.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/o3dr.h"
#include "../../include/o3dr_contour.h"
#include "../../include/o3dr_dem.h"
#include "../../include/o3dr_objects.h"
#include "../../include/o3dr_terrain.h"

namespace o3dr_host {

typedef o3dr_point PointXYZRGB;                 // 16 B: x,y,z + a<<24|r<<16|g<<8|b
typedef std::array<float, 16> Matrix4;          // row-major 4x4 (the reference's Eigen Matrix4f, by value)

struct PointCloud {                             // the slice of pcl::PointCloud the hot path uses
    typedef std::shared_ptr<PointCloud> Ptr;
    std::vector<PointXYZRGB> points;
    bool is_dense = true;
    size_t size() const { return points.size(); }
};

struct Image8 {                                 // cv::Mat stand-in: 8-bit, 1 or 3 interleaved channels (B,G,R)
    int rows = 0, cols = 0, channels = 0;
    std::vector<uint8_t> data;
    bool empty() const { return data.empty(); }
    int64_t pitch() const { return (int64_t)cols * channels; }
};

// ---- I/O helpers (png_io.cpp, ply_io.cpp) ------------------------------------------------------------
// cv::imread(path) / cv::imread(path, IMREAD_GRAYSCALE) for 8-bit non-interlaced PNGs; empty on failure
Image8 read_png(const std::string& path, bool grayscale);
struct Image16 {                                // one 16-bit channel: a segment label image
    int rows = 0, cols = 0;
    std::vector<uint16_t> data;
    bool empty() const { return data.empty(); }
};
// a label image: greyscale (colour type 0), 8 or 16 bits per sample, non-interlaced; empty on failure or any other format
Image16 read_png_labels(const std::string& path);
// an 8-bit greyscale PNG (stored deflate blocks: no compression); false if the file cannot be written
bool write_png_grey8(const std::string& path, const uint8_t* data, int rows, int cols);
// a 16-bit greyscale PNG (a segment label image, as read_png_labels reads it)
bool write_png_grey16(const std::string& path, const uint16_t* data, int rows, int cols);
// the same for an 8-bit interleaved B G R image (the file holds R G B, colour type 2)
bool write_png_bgr8(const std::string& path, const uint8_t* data, int rows, int cols);
// pcl::io::savePLYFileBinary layout (x,y,z float + r,g,b uchar, then one `camera` element); with normals (4 floats per
// point: nx ny nz curvature) PointXYZRGBNormal's (the same, then normal_x normal_y normal_z curvature float)
bool save_ply_binary(const std::string& path, const PointCloud& cloud, const std::vector<float>* normals = nullptr);
// pcl::PLYReader for binary little-endian files: x y z red green blue by name out of the vertex element (the files
// save_ply_binary writes, build/cloud.ply); false if one is missing or the vertex layout is not fixed-size
bool read_ply(const std::string& path, PointCloud& cloud);
// a triangle mesh as pcl::io::savePLYFileBinary writes a PolygonMesh: the vertices (x y z float + red green blue uchar, with
// normals (3 floats per point) also nx ny nz float), then `element face` with `property list uchar int vertex_indices`
bool save_ply_mesh(const std::string& path, const PointCloud& cloud, const std::vector<int32_t>& tris,
                   const std::vector<float>* normals = nullptr);

class RawImageData {  // pose.h:54-70
public:
    int img_num = 0;
    Image8 rgb_image, disparity_image;
    Image16 label_image;  // --use_segment_labels
    Image8 right_image;   // --gpu_disparity: the pair's right image; disparity_image is then o3dr_stereo_disparity's
    double time = 0, tx = 0, ty = 0, tz = 0, qx = 0, qy = 0, qz = 0, qw = 1;
};

class ImageData {  // pose.h:73-85 (the hot-path fields)
public:
    RawImageData* raw_img_data_ptr = nullptr;
    std::vector<float> keypoints_xy;  // features.keypoints pt.x,pt.y pairs, from --keypoints_dir; empty: none given
                                      // (--gpu_keypoints makes a batch's keypoints with o3dr_orb_detect instead)
    Matrix4 t_mat_MAVLink{}, t_mat_FeatureMatched{};
};

class Pose {
public:
    Pose(int argc, char* argv[]);  // like the reference, the whole program runs inside the constructor
    ~Pose();

    // ---- the `Pose` members the hot path reads, reference defaults (pose.h:92-175) --------------------
    double minDisparity = 64;
    int boundingBox = 20;
    int rows = 0, cols = 0, cols_start_aft_cutout = 0;
    int jump_pixels = 10;
    int seq_len = -1;
    int blur_kernel = 1;
    unsigned int min_points_per_voxel = 1;
    double voxel_size = 0.1;
    int cutout_ratio = 8;
    bool dont_downsample = false, downsample = false, log_stuff = false, only_MAVLink = true, dont_icp = true;
    bool reference_fanout = false;  // run A6 through createAndTransformPtCloud on 7 host threads
    bool sor = true;                // statistical outlier removal of the per-frame path (pose_functions.cpp:1673-1686:
                                    // always on in the reference when jump_pixels > 0); `--sor 0` switches it off
    std::string keypointsPrefix;    // --keypoints_dir: <img_num>.txt with one "x y" pair per line (KeyPoint::pt of the
                                    // frame's ORB features, e.g. the files --find_features writes); empty = no keypoints
    std::array<double, 16> Q{};
    std::string calib_file = "cam13calib.yml";
    std::string dataFilesPrefix = "data_files/", imagePrefix = "images/", disparityPrefix = "disparities/";
    std::string outputPrefix = "output/";
    std::string read_PLY_filename0, read_PLY_filename1;
    bool align_point_cloud = false;  // --align_point_cloud source.ply target.ply (pose.cpp:46-112): ICP through o3dr_icp_align
    int icp_max_iterations = 10;     // --icp_max_iterations (pcl::Registration defaults)
    double icp_max_corr_dist = HUGE_VAL, icp_transformation_epsilon = 0.0;  // --icp_max_corr_dist, --icp_transformation_epsilon
    bool smooth_surface = false;     // --smooth_surface file.ply (pose.cpp:27-112): MLS through o3dr_mls_smooth
    double search_radius = 0.0;      // --search_radius: required by --smooth_surface and --mesh_surface, ignored elsewhere
    bool search_radius_set = false;
    int mls_polynomial_order = 2;    // --mls_polynomial_order (PCL's default)
    double mls_sqr_gauss_param = 0.0;  // --mls_sqr_gauss_param (0: search_radius^2)
    bool mls_normals = false;        // --mls_normals: PointXYZRGBNormal output
    bool segment_cloud_only = false; // --segment_cloud_only file.ply (segmentCloud, pose_functions.cpp:2094-2249)
    double sac_distance_threshold = 0.0;  // --sac_distance_threshold: required by --segment_cloud_only
    bool sac_distance_threshold_set = false;
    int sac_max_iterations = 1000;   // --sac_max_iterations
    double segment_tile_size = 0.0;  // --segment_tile_size (0: one plane for the cloud)
    unsigned long long sac_seed = 0; // --sac_seed
    int sac_optimize = 1;            // --sac_optimize
    bool mesh_surface = false;       // --mesh_surface file.ply (pose.cpp:27-112, GP3): o3dr_mesh_surface
    bool mesh_normals = false;       // --mesh_normals: nx ny nz per vertex
    bool orthophoto = false;         // --orthophoto file.ply: o3dr_rasterize_map of one PLY -> ortho_ / height_ / shade_<file>.png
    std::string orthophoto_out;      // --orthophoto_out prefix (reconstruction run): the same three images of the final merged
                                     // cloud, as <prefix>ortho.png, <prefix>height.png and, with --ortho_light, <prefix>shade.png
    std::string ortho_select = "first";  // --ortho_select first|top|bottom, --ortho_fill_radius r (cells, 0..32), --ortho_light lx ly lz;
    int ortho_fill_radius = 0;           // parsed and ignored without --orthophoto / --orthophoto_out
    bool ortho_light_set = false;
    double ortho_light[3] = {0.0, 0.0, 0.0};
    bool ground_filter = false;      // --ground_filter file.ply: o3dr_ground_filter of one PLY -> terrain_ / objects_<file>, dtm_<file>.png
    int ground_max_window = 16;      // --ground_max_window r (cells, 1..128), --ground_window_base b, --ground_linear,
    int ground_window_base = 2;      // --ground_slope s, --ground_initial_distance m, --ground_max_distance m,
    bool ground_linear = false;      // --ground_fill_radius r (cells, 0..32); parsed and ignored without --ground_filter
    double ground_slope = 0.7, ground_initial_distance = 0.15, ground_max_distance = 10.0;
    int ground_fill_radius = 0;
    bool ground_interpolate = false; // --ground_interpolate: the DTM interpolated from the ground cells (o3dr_raster_interpolate),
    int ground_smooth = 2;           // --ground_smooth n (sweeps per level, 0..8); parsed and ignored without --ground_filter
    bool cluster_cloud = false;      // --cluster_cloud file.ply: o3dr_cluster_euclidean of one PLY -> clusters_ / unclustered_<file>,
    bool cluster_tolerance_set = false;  // clusters_<file>.txt; --cluster_tolerance t (metres, required there),
    double cluster_tolerance = 0.0;  // --cluster_min_size n, --cluster_max_size n; parsed and ignored without --cluster_cloud
    int cluster_min_size = 1, cluster_max_size = INT32_MAX;
    bool contours = false;           // --contours file.ply: o3dr_raster_contours of one PLY's terrain model -> contours_<file>.geojson;
    bool contour_interval_set = false;  // --contour_interval m (required there), --contour_base b, --contour_surface dtm|dsm,
    double contour_interval = 0.0, contour_base = 0.0;  // --contour_min_segments n; parsed and ignored without --contours
    std::string contour_surface = "dtm";
    int contour_min_segments = 1;
    int device_id = 0;
    int n_gpus = 1;                 // --gpus N: frames sharded over devices device_id .. device_id+N-1, one host thread and
                                    // one context each, merged through o3dr_merge_partitioned (RCCL)
    bool partitioned_merge = false; // --partitioned_merge: take that path with one GPU as well
    bool preview = false;           // --preview: after every cycle, the merged map so far -> <output_dir>/preview.ply
                                    // (pose.cpp:437-448, 638-674), folded incrementally (o3dr_finalize_incremental)

    bool use_segment_labels = false;  // --use_segment_labels: every batch's disparities go through o3dr_plane_fit_disparity
                                      // and are accumulated as CV_64F (single-GPU batched path, also with --preview)
    std::string segmentLabelsPrefix = "segmentlabels/";  // --segment_labels_dir: <img_num>.png, 8- or 16-bit greyscale
    int plane_min_pixels = 3;         // --plane_min_pixels
    double plane_max_mse = 0.0;       // --plane_max_mse (0: no gate)
    std::string find_features_png;    // --find_features image.png: ORB keypoints of one image (o3dr_orb_detect), printed per
                                      // level and written as <image>.keypoints.txt in the --keypoints_dir format
    bool gpu_keypoints = false;       // --gpu_keypoints: with jump_pixels != 1 and no --keypoints_dir, every batch's keypoints
                                      // come from o3dr_orb_detect on its rgb images (single-GPU batched path)
    int orb_n_features = 1500, orb_levels = 5, orb_fast_threshold = 20;  // --orb_n_features, --orb_levels, --orb_fast_threshold
    float orb_scale = 1.3f;           // --orb_scale
    bool feature_poses = false;       // --feature_poses: every cycle's frames go through o3dr_orb_detect, o3dr_keypoints_3d (camera
                                      // frame) and o3dr_pose_chain; a matched frame's t_mat_FeatureMatched is the chain's pose, a
                                      // rejected frame is left out of the cycle's accumulate call (single-GPU batched path)
    double dist_nearby = 2.0;         // --dist_nearby, --range_width: the chain's nearby-frame test (with --feature_poses only)
    int range_width = 8;
    int chain_min_matches = 30;       // --chain_min_matches
    double chain_max_rms = HUGE_VAL;  // --chain_max_rms (default: no gate)
    bool chain_ransac = false;        // --chain_ransac_threshold given: o3dr_pose_chain_robust filters every pair's correspondences
    double chain_ransac_threshold = 0.05;  // (metres), --chain_ransac_iterations, --chain_ransac_seed
    int chain_ransac_iterations = 256;
    uint64_t chain_ransac_seed = 0;
    bool refine_poses = false;        // --refine_poses (with --feature_poses): after each cycle's chain, o3dr_pose_graph_refine over the
                                      // cycle's matched frames and pairs, the history held; a free frame's pose becomes the refined one
    int refine_gn_iterations = 5;     // --refine_gn_iterations, --refine_cg_iterations, --refine_prior_weight
    int refine_cg_iterations = 32;
    double refine_prior_weight = 0.0;
    std::string stereo_left_png, stereo_right_png;  // --stereo_disparity left.png right.png: o3dr_stereo_disparity of one
                                      // rectified pair, written as <left>.disparity.png (8-bit grey)
    bool gpu_disparity = false;       // --gpu_disparity: every frame's disparity image comes from o3dr_stereo_disparity on
    std::string rightImagePrefix;     // image_dir/<n>.png and --right_image_dir d/<n>.png instead of --disparity_dir
                                      // (single-GPU batched path)
    int stereo_n_disparities = 256, stereo_min_disparity = 0, stereo_p1 = 10, stereo_p2 = 120;  // --stereo_* flags
    int stereo_paths = 8, stereo_uniqueness = 10, stereo_lr_max_diff = 1;
    // --stereo_median 0|3|5, --stereo_speckle_size n, --stereo_speckle_diff n: o3dr_disparity_filter of the disparity image
    // in --stereo_disparity, --gpu_disparity and --filter_disparity; parsed and ignored elsewhere
    int stereo_median = 0, stereo_speckle_size = 0, stereo_speckle_diff = 1;
    std::string rectify_calib;        // --rectify_calib f: an OpenCV YAML file with M1 (or K1) D1 R1 P1 M2 (or K2) D2 R2 P2.  Every
                                      // rgb_image (under --gpu_disparity every right_image too) is replaced by its rectified
                                      // version right after it is read; --stereo_disparity rectifies its pair first
    std::string rectify_left_png, rectify_right_png;  // --rectify_pair left.png right.png: o3dr_rectify_maps + o3dr_rectify_remap of one
                                      // pair, written as <left>.rectified.png and <right>.rectified.png
    int rectify_border = 0;           // --rectify_border b: what a tap outside the source reads (0..255)
    std::string filter_disparity_png;  // --filter_disparity in.png: the filter alone on an 8-bit grey PNG -> <in>.filtered.png
    std::string segment_image_png;    // --segment_image image.png: o3dr_segment_image of one image -> <image>.labels.png (16-bit grey)
    int segment_step = 16, segment_compactness = 20, segment_iterations = 5, segment_min_size = -1;  // --segment_step, --segment_compactness,
                                      // --segment_iterations, --segment_min_size (negative: step * step / 4)
    bool gpu_segment_labels = false;  // --gpu_segment_labels (under --use_segment_labels): every frame's label image comes from
                                      // o3dr_segment_image on its rgb image, with the --segment_* flags, instead of --segment_labels_dir
    bool segment_labels_dir_set = false;
    bool multiview_filter = false;    // --multiview_filter: every cycle's accepted frames go through o3dr_multiview_filter once the
                                      // cycle's poses are final (recorded, --feature_poses, --refine_poses) and before they are
                                      // accumulated; neighbours are chosen among that cycle's accepted frames (single-GPU batched path)
    bool multiview_fuse = false;      // --multiview_fuse: the same step through o3dr_multiview_fuse; the cycle's frames are then accumulated
                                      // as float64 levels (disparity_f64 for that call); with --multiview_filter it means fuse
    int mv_neighbors = 4;             // --mv_neighbors k, --mv_max_distance m: o3dr_nearby_frames; parsed and ignored without the flag
    double mv_max_distance = HUGE_VAL;
    double mv_tolerance = 1.0;        // --mv_tolerance t (levels), --mv_min_support n, --mv_max_violations n (-1: the majority rule)
    int mv_min_support = 1, mv_max_violations = -1;
    std::string print_label_png;      // --print_label_png f: rows, cols and the labels of f as text (checks the reader)

    std::vector<RawImageData> rawImageDataVec;
    std::vector<ImageData> acceptedImageDataVec;

    // ---- the four entry points (pose.h:198,199,216,231) ------------------------------------------------
    void createSingleImgPtCloud(int accepted_img_index, PointCloud::Ptr cloudrgb);
    void transformPtCloud(PointCloud::Ptr cloudrgb, PointCloud::Ptr transformed_cloudrgb, Matrix4 transform);
    PointCloud::Ptr downsamplePtCloud(PointCloud::Ptr& cloudrgb, bool combinedPtCloud);
    void createAndTransformPtCloud(int accepted_img_index, PointCloud::Ptr& cloudrgb_return);

    // ---- control plane around them ---------------------------------------------------------------------
    Matrix4 generateTmat(int current_idx);                 // pose_functions.cpp:1178-1356
    double getMean(const Image8& disp_img);                // pose_functions.cpp:987-1005
    double getVariance(const Image8& disp_img);            // pose_functions.cpp:1007-1028
    int parseCmdArgs(int argc, char** argv);               // pose_functions.cpp:70-307 (hot-path flags)
    void printUsage();
    void readCalibFile();                                  // pose_functions.cpp:467-476
    void readPoseFile();                                   // pose_functions.cpp:478-506
    void populateData();                                   // pose_functions.cpp:624-744
    int binarySearchImageTime(int l, int r, int imageNumber);
    int binarySearchUsingTime(const std::vector<double>& seq, int l, int r, double time);
    void save_pt_cloud_to_PLY_File(PointCloud::Ptr cloudrgb, std::string& writePath);
    PointCloud::Ptr read_PLY_File(std::string point_cloud_filename);

private:
    o3dr_ctx* ctx_for_this_thread();
    void push_params(o3dr_ctx* c);
    void run_reconstruction();
    // a reconstruction cycle (pose.cpp): the accept loop, then the accepted frames into cloud_big - by --reference_fanout, or
    // stacked in one FrameBatch and through the stages in this order, each handing on in the batch or the CycleState
    struct FrameBatch;
    struct F64Images;
    struct CycleState;
    void accept_cycle(int& current_idx, int cycle_len);
    void fanout_cycle(size_t first, size_t last, PointCloud& cloud_big_host);
    void accumulate_cycle(o3dr_ctx* c, size_t first, size_t last);
    void orb_stage(o3dr_ctx* c, FrameBatch& b, CycleState& s);         // --gpu_keypoints, --feature_poses
    void plane_fit_stage(o3dr_ctx* c, FrameBatch& b, CycleState& s);   // --use_segment_labels
    void pose_chain_stage(o3dr_ctx* c, FrameBatch& b, CycleState& s);  // --feature_poses, --chain_ransac_*, --refine_poses
    void keep_chained_frames(FrameBatch& b, CycleState& s);            // the chain's status lines, its rejected frames leave the batch
    void multiview_stage(o3dr_ctx* c, FrameBatch& b, CycleState& s);   // --multiview_filter, --multiview_fuse
    void write_preview(o3dr_ctx* c);                                   // --preview
    void merge_and_save(o3dr_ctx* c, PointCloud::Ptr cloud_big_host);  // cloud.ply, --orthophoto_out
    void run_sharded(PointCloud::Ptr cloud_small);  // --gpus N
    void run_align_point_cloud();                   // --align_point_cloud
    void run_smooth_surface();                      // --smooth_surface
    void run_segment_cloud();                       // --segment_cloud_only
    void run_mesh_surface();                        // --mesh_surface
    void run_orthophoto();                          // --orthophoto
    void run_ground_filter();                       // --ground_filter
    void run_cluster_cloud();                       // --cluster_cloud
    void run_contours();                            // --contours
    // the map's rasters of a host cloud (o3dr_raster_extent, o3dr_rasterize_map with the --ortho_* flags) as PNGs, rows in
    // descending cy (north up); shade_path is written with --ortho_light only.  Prints the box, the counts and the call time.
    void write_map_rasters(o3dr_ctx* c, const PointCloud& cloud, const std::string& ortho_path, const std::string& height_path,
                           const std::string& shade_path);
    void run_find_features();                       // --find_features
    void run_stereo_disparity();                    // --stereo_disparity
    void compute_gpu_disparities();                 // --gpu_disparity: fills every raw frame's disparity_image
    void run_filter_disparity();                    // --filter_disparity
    void run_segment_image();                       // --segment_image
    void compute_gpu_segment_labels();              // --gpu_segment_labels: fills every raw frame's label_image
    o3dr_segment_params segment_params(int channels) const;  // the --segment_* flags over the defaults
    void readRectifyCalib();                        // --rectify_calib: fills rectify_cam (no device needed)
    void run_rectify_pair();                        // --rectify_pair
    void rectify_raw_images();                      // --rectify_calib in a reconstruction run: replaces the images read
    // o3dr_rectify_remap of images of one size (3 channels) through camera cam's map (0: left, 1: right) of that size, in
    // place, one call; n_valid: the map's valid-pixel count, or nullptr
    void rectify_images(o3dr_ctx* c, int cam, const std::vector<Image8*>& imgs, int64_t* n_valid);
    bool disparity_filter_on() const { return stereo_median != 0 || stereo_speckle_size > 0; }
    // o3dr_disparity_filter of n_frames tight uint8 images in place, with the three flags; info: one per frame, or nullptr
    void filter_disparities(o3dr_ctx* c, std::vector<uint8_t>& disp, int rows, int cols, int n_frames, o3dr_disparity_filter_info* info);
    o3dr_stereo_params stereo_params(int channels) const;  // the --stereo_* flags over the defaults
    o3dr_orb_params orb_params() const;             // the --orb_* flags over the defaults
    int first_img_num = -1, last_img_num = -1;
    bool run3d_reconstruction = true;
    // --feature_poses: the frames already through the chain (descriptors, camera-frame keypoints, row offsets, recorded
    // poses, the chain's poses and statuses): the history of the next cycle's o3dr_pose_chain call
    struct ChainHistory {
        std::vector<uint8_t> desc;
        std::vector<o3dr_point> kp3;
        std::vector<int64_t> off{0};
        std::vector<float> prior, poses;
        std::vector<int32_t> status;
    } chain;
    o3dr_rectify_camera rectify_cam[2] = {};  // --rectify_calib: the left and the right camera
    struct RectifyMap {          // a camera's map at the size it was last asked for
        int rows = 0, cols = 0;
        std::vector<int32_t> map;
    } rectify_map[2];
    bool disparity_f64 = false;  // what push_params sets: on while a cycle's F64Images lives (plane fits, fused levels)
    std::vector<std::vector<double>> pose_data, images_times_data;
    std::vector<double> pose_times_seq, images_times_seq;
    std::ofstream log_file;
    std::vector<o3dr_ctx*> all_ctx;
};

}  // namespace o3dr_host
