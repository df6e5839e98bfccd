// pose.cpp — host side of the hot path: the reference's `Pose` entry points on top of libo3dr.
// Reference lines restated are cited at each function (paths relative to the reference tree).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iomanip>
#include <iostream>
#include <mutex>
#include <optional>
#include <sstream>
#include <stdexcept>
#include <thread>

#include "o3dr_host.h"

using namespace std;

namespace o3dr_host {

static void chk(int rc, const char* what)
{
    if (rc != O3DR_OK) throw runtime_error(string(what) + ": " + o3dr_last_error());
}

static const char* const kChainStatusName[] = {"ANCHOR", "MATCHED", "TOO_FEW", "DEGENERATE", "RMS"};             // O3DR_CHAIN_*
static const char* const kIcpReasonName[] = {"MAX_ITERATIONS", "UNCHANGED", "SMALL_STEP", "TOO_FEW", "DEGENERATE"};  // o3dr_icp_result.reason

// <dir>/<prefix><file><suffix> next to path = <dir>/<file>: where a tool writes what it made of that file
static string next_to(const string& path, const string& prefix, const string& suffix = string())
{
    const size_t cut = path.find_last_of('/') == string::npos ? 0 : path.find_last_of('/') + 1;
    return path.substr(0, cut) + prefix + path.substr(cut) + suffix;
}

static void warn_voxel_overflow(uint32_t status)  // PCL_WARN of VoxelGrid::applyFilter
{
    if (status & O3DR_STATUS_VOXEL_OVERFLOW)
        cerr << "[pcl::VoxelGrid::applyFilter] Leaf size is too small for the input dataset. Integer indices would overflow." << endl;
}

// ------------------------------------------------------------------------------------------------
// contexts: the reference calls createAndTransformPtCloud from up to 7 threads (pose.cpp:392-413);
// a libo3dr context is single-threaded, so each calling thread gets its own.
// ------------------------------------------------------------------------------------------------
static mutex g_ctx_mu;
static thread_local o3dr_ctx* tl_ctx = nullptr;

o3dr_ctx* Pose::ctx_for_this_thread()
{
    if (!tl_ctx) {
        chk(o3dr_ctx_create(device_id, &tl_ctx), "o3dr_ctx_create");
        lock_guard<mutex> lk(g_ctx_mu);
        all_ctx.push_back(tl_ctx);
    }
    push_params(tl_ctx);
    return tl_ctx;
}

void Pose::push_params(o3dr_ctx* c)
{
    o3dr_params p;
    o3dr_default_params(&p);
    p.min_disparity = minDisparity;
    p.voxel_size = voxel_size;
    p.bounding_box = boundingBox;
    p.cutout_ratio = cutout_ratio;
    p.jump_pixels = jump_pixels;
    p.min_points_per_voxel = min_points_per_voxel;
    p.dont_downsample = dont_downsample ? 1 : 0;
    p.sor_enable = sor ? 1 : 0;
    p.blur_kernel = blur_kernel;  // > 1: bilateral filter on the disparity image first (pose_functions.cpp:1040-1047)
    p.disparity_f64 = disparity_f64 ? 1 : 0;  // --use_segment_labels: the plane-fitted CV_64F image (pose_functions.cpp:1037,1102)
    chk(o3dr_set_params(c, &p), "o3dr_set_params");
    chk(o3dr_set_camera(c, Q.data()), "o3dr_set_camera");
}

Pose::~Pose()
{
    for (o3dr_ctx* c : all_ctx) o3dr_ctx_destroy(c);
    if (tl_ctx) tl_ctx = nullptr;
}

// ------------------------------------------------------------------------------------------------
// the four entry points
// ------------------------------------------------------------------------------------------------
// pose.h:198 / pose_functions.cpp:1030-1134
void Pose::createSingleImgPtCloud(int accepted_img_index, PointCloud::Ptr cloudrgb)
{
    cloudrgb->is_dense = true;
    const ImageData& im = acceptedImageDataVec[accepted_img_index];
    const RawImageData& raw = *im.raw_img_data_ptr;
    o3dr_ctx* c = ctx_for_this_thread();
    const int n_kp = (int)(im.keypoints_xy.size() / 2);
    const int64_t cap = o3dr_max_points(c, rows, cols) + n_kp;
    cloudrgb->points.resize((size_t)(cap > 0 ? cap : 1));
    int64_t n = 0;
    chk(o3dr_create_single_img_pt_cloud(c, raw.disparity_image.data.data(), raw.disparity_image.pitch(),
                                        raw.rgb_image.data.data(), raw.rgb_image.pitch(), rows, cols,
                                        n_kp ? im.keypoints_xy.data() : nullptr, n_kp, cloudrgb->points.data(), cap, &n,
                                        O3DR_MEM_HOST),
        "createSingleImgPtCloud");
    cloudrgb->points.resize((size_t)n);
    cout << " " << raw.img_num << std::flush;  // :1131-1133
    if (log_file.is_open()) log_file << " " << raw.img_num << "/" << cloudrgb->points.size() << std::flush;
}

// pose.h:199 / pose_functions.cpp:1358-1362
void Pose::transformPtCloud(PointCloud::Ptr cloudrgb, PointCloud::Ptr transformed_cloudrgb, Matrix4 transform)
{
    transformed_cloudrgb->points.resize(cloudrgb->points.size());
    transformed_cloudrgb->is_dense = cloudrgb->is_dense;
    chk(o3dr_transform_pt_cloud(ctx_for_this_thread(), cloudrgb->points.data(), (int64_t)cloudrgb->points.size(),
                                transform.data(), transformed_cloudrgb->points.data(), O3DR_MEM_HOST),
        "transformPtCloud");
}

// pose.h:216 / pose_functions.cpp:1654-1709
PointCloud::Ptr Pose::downsamplePtCloud(PointCloud::Ptr& cloudrgb, bool combinedPtCloud)
{
    PointCloud::Ptr out(new PointCloud());
    const int64_t n_in = (int64_t)cloudrgb->points.size();
    out->points.resize((size_t)(n_in > 0 ? n_in : 1));
    int64_t n = 0;
    uint32_t status = 0;
    chk(o3dr_downsample_pt_cloud(ctx_for_this_thread(), cloudrgb->points.data(), n_in, combinedPtCloud ? 1 : 0,
                                 out->points.data(), n_in > 0 ? n_in : 1, &n, &status, O3DR_MEM_HOST),
        "downsamplePtCloud");
    warn_voxel_overflow(status);
    out->points.resize((size_t)n);
    return out;
}

// pose.h:231 / pose.cpp:596-636: every exception is caught and printed, the output cloud is left empty
void Pose::createAndTransformPtCloud(int accepted_img_index, PointCloud::Ptr& cloudrgb_return)
{
    try {
        const ImageData& im = acceptedImageDataVec[accepted_img_index];
        const RawImageData& raw = *im.raw_img_data_ptr;
        o3dr_ctx* c = ctx_for_this_thread();
        const int n_kp = (int)(im.keypoints_xy.size() / 2);
        const int64_t cap = o3dr_max_points(c, rows, cols) + n_kp;
        cloudrgb_return->points.resize((size_t)(cap > 0 ? cap : 1));
        int64_t n = 0;
        uint32_t status = 0;
        const int rc = o3dr_create_and_transform_pt_cloud(
            c, raw.disparity_image.data.data(), raw.disparity_image.pitch(), raw.rgb_image.data.data(),
            raw.rgb_image.pitch(), rows, cols, im.t_mat_FeatureMatched.data(), n_kp ? im.keypoints_xy.data() : nullptr, n_kp,
            cloudrgb_return->points.data(), cap, &n, &status, O3DR_MEM_HOST);
        cloudrgb_return->points.resize((size_t)(rc == O3DR_OK ? n : 0));
        if (rc != O3DR_OK) throw runtime_error(o3dr_last_error());
        cout << " " << raw.img_num << std::flush;
        if (log_file.is_open()) log_file << " " << raw.img_num << "/" << n << std::flush;
    } catch (const std::exception& e) {
        cout << "Exception caught in thread with accepted_img_index=" << accepted_img_index << endl;
        cout << e.what() << endl;
        cloudrgb_return->points.clear();
    } catch (...) {
        cout << "General Exception caught in thread with accepted_img_index=" << accepted_img_index << endl;
        cloudrgb_return->points.clear();
    }
}

// ------------------------------------------------------------------------------------------------
// control plane: pose matrix, gates, readers
// ------------------------------------------------------------------------------------------------
static Matrix4 mul4(const Matrix4& a, const Matrix4& b)
{  // float 4x4 product, each coefficient ((a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j) + a_i3 b_3j
    Matrix4 o{};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float s = a[i * 4] * b[j];
            for (int k = 1; k < 4; ++k) s = s + a[i * 4 + k] * b[k * 4 + j];
            o[i * 4 + j] = s;
        }
    return o;
}
static Matrix4 ident()
{
    Matrix4 m{};
    m[0] = m[5] = m[10] = m[15] = 1.f;
    return m;
}

// pose_functions.cpp:1178-1356: camera mounting (pose.h:142-147) x quaternion x translation, as float
// 4x4 factors multiplied left to right (:1341).  Eigen may order/fuse the inner sums differently from
// this plain loop (agreement ~1e-6).
Matrix4 Pose::generateTmat(int current_idx)
{
    const double PI = 3.141592653589793238463;
    const double theta_xi = -1.1408 * PI / 180, theta_yi = 1.1945 * PI / 180;
    const double trans_x_hi = -0.300, trans_y_hi = -0.040, trans_z_hi = -0.350;
    Matrix4 r_xi = ident();
    r_xi[5] = (float)cos(theta_xi); r_xi[6] = (float)-sin(theta_xi); r_xi[9] = (float)sin(theta_xi); r_xi[10] = (float)cos(theta_xi);
    Matrix4 r_yi = ident();
    r_yi[0] = (float)cos(theta_yi); r_yi[2] = (float)sin(theta_yi); r_yi[8] = (float)-sin(theta_yi); r_yi[10] = (float)cos(theta_yi);
    Matrix4 r_invert_i = ident();
    r_invert_i[5] = -1.f; r_invert_i[10] = -1.f;
    Matrix4 r_invert_y = ident();
    r_invert_y[5] = -1.f;
    Matrix4 t_hi = ident();
    t_hi[3] = (float)trans_x_hi; t_hi[7] = (float)trans_y_hi; t_hi[11] = (float)trans_z_hi;
    Matrix4 r_flip_xy{};
    r_flip_xy[4] = 1.f; r_flip_xy[1] = 1.f; r_flip_xy[10] = 1.f; r_flip_xy[15] = 1.f;

    const RawImageData& r = rawImageDataVec[current_idx];
    const double qx = r.qx, qy = r.qy, qz = r.qz, qw = r.qw;
    const double sqw = qw * qw, sqx = qx * qx, sqy = qy * qy, sqz = qz * qz;
    if (sqw + sqx + sqy + sqz < 0.99 || sqw + sqx + sqy + sqz > 1.01)
        throw "Exception: Sum of squares of quaternion values should be 1! i.e., quaternion should be homogeneous!";
    double rot[3][3];
    rot[0][0] = sqx - sqy - sqz + sqw;
    rot[1][1] = -sqx + sqy - sqz + sqw;
    rot[2][2] = -sqx - sqy + sqz + sqw;
    double t1 = qx * qy, t2 = qz * qw;
    rot[0][1] = 2.0 * (t1 + t2);
    rot[1][0] = 2.0 * (t1 - t2);
    t1 = qx * qz; t2 = qy * qw;
    rot[0][2] = 2.0 * (t1 - t2);
    rot[2][0] = 2.0 * (t1 + t2);
    t1 = qy * qz; t2 = qx * qw;
    rot[1][2] = 2.0 * (t1 + t2);
    rot[2][1] = 2.0 * (t1 - t2);
    Matrix4 r_wh = ident();
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r_wh[i * 4 + j] = (float)rot[j][i];  // rot = rot.t()
    Matrix4 t_wh = ident();
    t_wh[3] = (float)r.tx; t_wh[7] = (float)r.ty; t_wh[11] = (float)r.tz;
    Matrix4 m = t_wh;
    const Matrix4* chain[] = {&r_wh, &r_invert_y, &r_flip_xy, &t_hi, &r_invert_i, &r_yi, &r_xi};
    for (const Matrix4* f : chain) m = mul4(m, *f);
    return m;
}

// pose_functions.cpp:987-1005
double Pose::getMean(const Image8& disp_img)
{
    double sum = 0.0;
    for (int y = boundingBox; y < rows - boundingBox; ++y)
        for (int x = cols_start_aft_cutout; x < cols - boundingBox; ++x) {
            const double d = (double)disp_img.data[(size_t)y * disp_img.cols + x];
            if (d > minDisparity) sum += d;
        }
    return sum / ((rows - 2 * boundingBox) * (cols - boundingBox - cols_start_aft_cutout));
}
// pose_functions.cpp:1007-1028
double Pose::getVariance(const Image8& disp_img)
{
    const double mean = getMean(disp_img);
    double temp = 0;
    for (int y = boundingBox; y < rows - boundingBox; ++y)
        for (int x = cols_start_aft_cutout; x < cols - boundingBox; ++x) {
            const double d = (double)disp_img.data[(size_t)y * disp_img.cols + x];
            if (d > minDisparity) temp += (d - mean) * (d - mean);
        }
    return temp / ((rows - 2 * boundingBox) * (cols - boundingBox - cols_start_aft_cutout) - 1);
}

// CSV of doubles, one record per line (pose_functions.cpp:351-397)
static vector<vector<double>> read_csv(const string& path)
{
    ifstream f(path);
    if (!f.is_open()) throw runtime_error("Exception: Could not open " + path);
    vector<vector<double>> data;
    string line;
    while (getline(f, line)) {
        vector<double> rec;
        stringstream ss(line);
        string field;
        while (getline(ss, field, ',')) rec.push_back(strtod(field.c_str(), nullptr));
        data.push_back(rec);
    }
    return data;
}

// pose_functions.cpp:402-426
int Pose::binarySearchImageTime(int l, int r, int imageNumber)
{
    while (r >= l) {
        const int mid = l + (r - l) / 2;
        const int v = (int)images_times_data[mid][0];
        if (v == imageNumber) return mid;
        if (v > imageNumber) r = mid - 1; else l = mid + 1;
    }
    throw "Exception: binarySearchImageTime: unsuccessful search!";
}
// pose_functions.cpp:431-465: returns an index whose NEIGHBOURS bracket `time`
int Pose::binarySearchUsingTime(const vector<double>& seq, int l, int r, double time)
{
    while (r >= l) {
        const int mid = l + (r - l) / 2;
        if (mid > 0 && mid < (int)seq.size() - 1) {
            if (seq[mid - 1] < time && seq[mid + 1] > time) return mid;
        } else if (mid == 0) {
            return 0;
        } else {
            return (int)seq.size() - 1;
        }
        if (seq[mid] > time) r = mid - 1; else l = mid + 1;
    }
    throw "Exception: binarySearchUsingTime: unsuccessful search!";
}

// The numbers of `<key>: !!opencv-matrix ... data: [ ... ]` in the text of an OpenCV YAML file, in file order; false if the
// entry or its data is missing.  The key is looked for at the start of a line (the last "key:" anywhere, if there is none).
static bool yaml_matrix_data(const string& txt, const string& key, vector<double>& out)
{
    size_t p = txt.find("\n" + key + ":");
    if (p == string::npos) p = txt.rfind(key + ":");
    if (p == string::npos) return false;
    p = txt.find("data:", p);
    if (p == string::npos) return false;
    const size_t a = txt.find('[', p);
    const size_t b = a == string::npos ? a : txt.find(']', a);
    if (a == string::npos || b == string::npos) return false;
    string body = txt.substr(a + 1, b - a - 1);
    for (char& ch : body)
        if (ch == ',' || ch == '\n') ch = ' ';
    stringstream vs(body);
    out.clear();
    string tok;
    while (vs >> tok) {
        char* end = nullptr;
        const double v = strtod(tok.c_str(), &end);
        if (end == tok.c_str() || *end) return false;
        out.push_back(v);
    }
    return true;
}

// pose_functions.cpp:467-476 — `Q: !!opencv-matrix ... data: [ 16 doubles ]` of an OpenCV YAML file
void Pose::readCalibFile()
{
    ifstream f(dataFilesPrefix + calib_file);
    if (!f.is_open()) throw "Exception: could not read Q matrix";
    stringstream ss;
    ss << f.rdbuf();
    vector<double> v;
    if (!yaml_matrix_data(ss.str(), "Q", v) || v.size() < 16) throw "Exception: could not read Q matrix";
    for (int i = 0; i < 16; ++i) Q[i] = v[(size_t)i];
    cout << "read calib file." << endl;
}

// --rectify_calib: the eight matrices stereoCalibrate + stereoRectify leave in one OpenCV YAML file - M1 D1 R1 P1 for the
// left camera, M2 D2 R2 P2 for the right one (K1 / K2 are taken for M1 / M2); D of 4, 5 or 8 entries.  Host only.
void Pose::readRectifyCalib()
{
    ifstream f(rectify_calib);
    if (!f.is_open()) throw runtime_error("--rectify_calib: could not read " + rectify_calib);
    stringstream ss;
    ss << f.rdbuf();
    const string txt = ss.str();
    for (int k = 0; k < 2; ++k) {
        const string n = to_string(k + 1);
        o3dr_rectify_camera& cam = rectify_cam[k];
        auto take = [&](const string& key, const string& alt, double* dst, size_t count) {
            vector<double> v;
            if (!yaml_matrix_data(txt, key, v) && (alt.empty() || !yaml_matrix_data(txt, alt, v)))
                throw runtime_error("--rectify_calib: " + rectify_calib + " has no matrix " + key);
            if (v.size() != count)
                throw runtime_error("--rectify_calib: " + key + " must have " + to_string(count) + " entries, has " + to_string(v.size()));
            copy(v.begin(), v.end(), dst);
        };
        take("M" + n, "K" + n, cam.K, 9);
        take("R" + n, "", cam.R, 9);
        take("P" + n, "", cam.P, 12);
        vector<double> d;
        if (!yaml_matrix_data(txt, "D" + n, d)) throw runtime_error("--rectify_calib: " + rectify_calib + " has no matrix D" + n);
        if (d.size() != 4 && d.size() != 5 && d.size() != 8)
            throw runtime_error("--rectify_calib: D" + n + " must have 4, 5 or 8 entries, has " + to_string(d.size()));
        fill(cam.D, cam.D + 8, 0.0);
        copy(d.begin(), d.end(), cam.D);
    }
}

// pose_functions.cpp:478-506
void Pose::readPoseFile()
{
    pose_data = read_csv(dataFilesPrefix + "pose.txt");
    pose_times_seq.clear();
    for (auto& r : pose_data) pose_times_seq.push_back(r.size() > 2 ? r[2] : 0.0);
    images_times_data = read_csv(dataFilesPrefix + "images.txt");
    images_times_seq.clear();
    for (auto& r : images_times_data) images_times_seq.push_back(r.size() > 2 ? r[2] : 0.0);
    cout << "Your images_times file contains " << images_times_data.size() << " records.\n";
    cout << "Your pose_data file contains " << pose_data.size() << " records.\n";
}

// pose_functions.cpp:624-744: the reference spreads imread over 7+7 threads; so does this
void Pose::populateData()
{
    readCalibFile();
    if (log_stuff) log_file.open(outputPrefix + "log.txt", ios::out);
    const int n = (int)rawImageDataVec.size();
    const int n_threads = 7;
    vector<thread> pool;
    mutex mu;
    for (int t = 0; t < n_threads; ++t)
        pool.emplace_back([&, t]() {
            for (int i = t; i < n; i += n_threads) {
                RawImageData& r = rawImageDataVec[i];
                r.rgb_image = read_png(imagePrefix + to_string(r.img_num) + ".png", false);       // :523-536
                if (gpu_disparity)  // the disparity image is made after the reads, from the pair (compute_gpu_disparities)
                    r.right_image = read_png(rightImagePrefix + to_string(r.img_num) + ".png", false);
                else
                    r.disparity_image = read_png(disparityPrefix + to_string(r.img_num) + ".png", true);  // :546-585
                if (use_segment_labels && !gpu_segment_labels) {  // (--gpu_segment_labels: made after the reads, compute_gpu_segment_labels)
                    r.label_image = read_png_labels(segmentLabelsPrefix + to_string(r.img_num) + ".png");
                    if (!r.disparity_image.empty() &&
                        (r.label_image.rows != r.disparity_image.rows || r.label_image.cols != r.disparity_image.cols))
                        r.label_image = Image16();  // (a label image of another size is no label image for this frame)
                }
                try {
                    const int it = binarySearchImageTime(0, (int)images_times_seq.size() - 1, r.img_num);
                    const int ip = binarySearchUsingTime(pose_times_seq, 0, (int)pose_times_seq.size() - 1, images_times_seq[it]);
                    r.time = images_times_seq[it];
                    const vector<double>& p = pose_data[ip];  // pose.h:140 tx_ind=3 .. qw_ind=9
                    r.tx = p[3]; r.ty = p[4]; r.tz = p[5]; r.qx = p[6]; r.qy = p[7]; r.qz = p[8]; r.qw = p[9];
                } catch (...) {
                    lock_guard<mutex> lk(mu);
                    cout << " no_pose_for_" << r.img_num << " " << flush;
                    r.disparity_image = Image8();
                    r.right_image = Image8();
                }
                lock_guard<mutex> lk(mu);
                cout << (r.rgb_image.empty() ? " cannot_read_i" : " i") << r.img_num
                     << ((gpu_disparity ? r.right_image.empty() : r.disparity_image.empty()) ? " cannot_read_d" : " d")
                     << r.img_num << " " << flush;
            }
        });
    for (thread& t : pool) t.join();
    cout << endl;
    if (!rectify_calib.empty()) rectify_raw_images();  // before anything else sees the images
    if (gpu_disparity) compute_gpu_disparities();
    if (use_segment_labels && gpu_segment_labels) compute_gpu_segment_labels();  // where the PNGs would have been read
    for (const RawImageData& r : rawImageDataVec)
        if (!r.disparity_image.empty()) {  // rows/cols from the first readable image (:635-638)
            rows = r.disparity_image.rows;
            cols = r.disparity_image.cols;
            cols_start_aft_cutout = (int)(cols / cutout_ratio);
            break;
        }
}

void Pose::save_pt_cloud_to_PLY_File(PointCloud::Ptr cloudrgb, string& writePath)
{
    if (!save_ply_binary(writePath, *cloudrgb)) throw runtime_error("could not write " + writePath);
    cerr << "Saved Point Cloud with " << cloudrgb->points.size() << " data points to " << writePath << endl;
}
PointCloud::Ptr Pose::read_PLY_File(string point_cloud_filename)
{
    cout << "Reading PLY file..." << endl;
    PointCloud::Ptr c(new PointCloud());
    if (!read_ply(point_cloud_filename, *c)) throw runtime_error("could not read " + point_cloud_filename);
    cout << "Read PLY file!" << endl;
    return c;
}

// ------------------------------------------------------------------------------------------------
// CLI (pose_functions.cpp:3-307): the hot-path flags keep their names and meaning; the three data
// directories, hard-coded absolute paths in the reference (pose.h:134-137), are flags here.
// ------------------------------------------------------------------------------------------------
void Pose::printUsage()
{
    cout << "./pose first_img last_img [--voxel_size m] [--jump_pixels n] [--min_points_per_voxel n] [--seq_len n]\n"
            "       [--dont_downsample] [--log 0|1] [--only_MAVLink] [--dont_icp] [--reference_fanout] [--sor 0|1]\n"
            "       [--data_dir d/] [--image_dir d/] [--disparity_dir d/] [--output_dir d/] [--calib_file f] [--device n]\n"
            "       [--keypoints_dir d/]   (d/<img_num>.txt: one \"x y\" keypoint per line; used iff jump_pixels != 1)\n"
            "       [--gpus N]   (frames sharded over N GPUs from --device on, one host thread each; the final merge is exchanged\n"
            "                     over RCCL and equals the one-GPU result bit for bit)  [--partitioned_merge]  (same path, N = 1)\n"
            "       [--preview]  (after every cycle of --seq_len frames: the merged cloud so far -> output_dir/preview.ply,\n"
            "                     folding only the new points; single-GPU batched path only)\n"
            "--sor defaults to 1: like the reference, every per-frame cloud goes through StatisticalOutlierRemoval(50, 1.0)\n"
            "before its voxel grid when jump_pixels > 0.\n"
            "./pose --downsample file.ply [--voxel_size m] [--min_points_per_voxel n]\n"
            "./pose --align_point_cloud source.ply target.ply [--icp_max_iterations n] [--icp_max_corr_dist m]\n"
            "       [--icp_transformation_epsilon e]   (point-to-point ICP of source onto target: prints T, fitness, correspondences,\n"
            "                     iterations and the reason it stopped; writes the source moved by T as aligned_<source> next to\n"
            "                     it - that file name is this build's own)\n"
            "./pose --smooth_surface file.ply --search_radius r [--mls_polynomial_order 0|1|2] [--mls_sqr_gauss_param h]\n"
            "       [--mls_normals]   (moving-least-squares smoothing: writes the fitted points, in input order, as\n"
            "                     smoothed_<file> next to it - that file name is this build's own; --search_radius is required\n"
            "                     here; --mls_normals adds normal_x normal_y normal_z curvature per point)\n"
            "--search_radius is ignored in every mode but --smooth_surface and --mesh_surface.\n"
            "./pose --segment_cloud_only file.ply --sac_distance_threshold t [--sac_max_iterations n] [--segment_tile_size m]\n"
            "       [--sac_seed s] [--sac_optimize 0|1]   (RANSAC plane per XY tile of m metres, 0 = one plane for the cloud:\n"
            "                     writes the inliers projected onto their tile's plane as ground_<file> and the rest as\n"
            "                     nonground_<file>, both in input order, next to it - those file names are this build's own;\n"
            "                     --sac_distance_threshold is required)\n"
            "./pose --mesh_surface file.ply --search_radius L [--voxel_size m] [--mesh_normals]   (height-field triangulation of\n"
            "                     the occupied XY cells of size m, edges up to L: writes every point, in input order, and the\n"
            "                     triangles as mesh_<file> next to it - that file name is this build's own; --search_radius is\n"
            "                     required here; --mesh_normals adds nx ny nz per vertex)\n"
            "./pose --orthophoto file.ply [--voxel_size m] [--ortho_select first|top|bottom] [--ortho_fill_radius r] [--ortho_light lx ly lz]\n"
            "                     (the map as images, one pixel per XY cell of size m, north up: the colours as ortho_<file>.png\n"
            "                     (8-bit B G R), the heights as height_<file>.png (16-bit grey, 0 = no data, else 1 + (z - z_min) / step)\n"
            "                     and, with --ortho_light, the shaded relief as shade_<file>.png, next to the source; a cell shows\n"
            "                     its first, highest or lowest point, an empty cell the nearest occupied one within r cells (0..32,\n"
            "                     default 0); prints the box, the counts, z_min, step and the call time - the flags and the file\n"
            "                     names are this build's own)\n"
            "       [--orthophoto_out prefix]  (reconstruction run: the same images of the final merged cloud, after cloud.ply, as\n"
            "                     <prefix>ortho.png, <prefix>height.png and <prefix>shade.png; not available with --gpus N > 1,\n"
            "                     --partitioned_merge, --reference_fanout; elsewhere the --ortho_* flags are parsed and ignored)\n"
            "./pose --ground_filter file.ply [--voxel_size m] [--ground_max_window r] [--ground_window_base b] [--ground_linear]\n"
            "       [--ground_slope s] [--ground_initial_distance m] [--ground_max_distance m] [--ground_fill_radius r]\n"
            "       [--ground_interpolate] [--ground_smooth n]\n"
            "                     (bare-earth ground filter on the XY cells of size m: the minimum surface is opened with windows\n"
            "                     growing to r cells (1..128, default 16) by powers of b (default 2) or, with --ground_linear, by\n"
            "                     steps of b, and a cell rising above the opening by more than s (default 0.7) times the window's\n"
            "                     growth in metres plus --ground_initial_distance (default 0.15), at most --ground_max_distance\n"
            "                     (default 10), is removed; writes the ground points as terrain_<file> and the others as\n"
            "                     objects_<file>, both in input order, and the terrain model as dtm_<file>.png (16-bit grey, north\n"
            "                     up, 0 = no data, else 1 + (z - z_min) / step; cells that are not ground take the nearest ground\n"
            "                     cell within --ground_fill_radius cells, 0..32, default 0) next to the source; prints the box, the\n"
            "                     schedule, the removed cells per iteration, the ground cells and points and the call time;\n"
            "                     with --ground_interpolate (and --ground_fill_radius 0) the terrain model is interpolated from the\n"
            "                     ground cells at any distance instead, pull-push over an image pyramid with n (0..8, default 2)\n"
            "                     smoothing sweeps per level: the picture has no 0 pixel, and the data cells, the filled cells and\n"
            "                     the pyramid's levels are printed;\n"
            "                     elsewhere the --ground_* flags are parsed and ignored - the flags and the file names are this\n"
            "                     build's own)\n"
            "./pose --cluster_cloud file.ply --cluster_tolerance t [--cluster_min_size n] [--cluster_max_size n]\n"
            "                     (Euclidean clustering: points closer than t metres are linked, a component of the links' closure\n"
            "                     with n_min <= points <= n_max (defaults 1 and 2^31 - 1) is a cluster, numbered by its lowest point\n"
            "                     index; writes the clustered points as clusters_<file>, cluster by cluster with a colour per\n"
            "                     cluster, the other points as unclustered_<file> in input order, and clusters_<file>.txt, one line\n"
            "                     per cluster: number first size lo[3] hi[3] centroid[3]; prints the counters, the first ten\n"
            "                     records and the call time; objects_<file> of --ground_filter is the intended input; elsewhere\n"
            "                     the --cluster_* flags are parsed and ignored - the flags and the file names are this build's own)\n"
            "./pose --contours file.ply --contour_interval m [--contour_base b] [--voxel_size m] [--contour_surface dtm|dsm]\n"
            "       [--contour_min_segments n]\n"
            "                     (contour lines at the elevations b + k m (b default 0) of the terrain model on the XY cells of\n"
            "                     --voxel_size: dtm (the default) is the ground filter's interpolated terrain model, --ground_filter\n"
            "                     --ground_interpolate at their defaults; dsm is the raster of every cell's highest point as it is,\n"
            "                     where lines end at holes; writes contours_<file>.geojson next to the source, a FeatureCollection\n"
            "                     with one LineString per line of at least n segments (default 1), in line order, with the\n"
            "                     properties line, level (k), elevation, closed and segments; prints the box, the level range, the\n"
            "                     counts and the call time; elsewhere the --contour_* flags are parsed and ignored - the flags and\n"
            "                     the file name are this build's own)\n"
            "./pose --find_features image.png [--orb_n_features n] [--orb_levels n] [--orb_scale s] [--orb_fast_threshold t]\n"
            "                     (ORB keypoints of one image: prints the count per level and writes one \"x y\" per line as\n"
            "                     <image>.keypoints.txt, the --keypoints_dir format - the flags and the file name are this build's own)\n"
            "       [--gpu_keypoints]  (reconstruction run with jump_pixels != 1 and no --keypoints_dir: every batch's keypoints come\n"
            "                     from the same extractor on its rgb images, with the --orb_* flags; single-GPU batched path only)\n"
            "./pose --stereo_disparity left.png right.png [--stereo_n_disparities n] [--stereo_min_disparity n] [--stereo_p1 n]\n"
            "       [--stereo_p2 n] [--stereo_paths 4|8] [--stereo_uniqueness n] [--stereo_lr_max_diff n]\n"
            "                     (census semi-global matching of one rectified pair: writes the 8-bit disparity image, 0 = rejected,\n"
            "                     as <left>.disparity.png and prints the accepted pixels and the call time - the flags and the file\n"
            "                     name are this build's own)\n"
            "       [--stereo_median 0|3|5] [--stereo_speckle_size n] [--stereo_speckle_diff n]  (the disparity image then goes\n"
            "                     through a k x k median and loses its connected components of at most n pixels, neighbours\n"
            "                     joined when they differ by at most --stereo_speckle_diff (default 1); also under --gpu_disparity)\n"
            "./pose --rectify_pair left.png right.png --rectify_calib f [--rectify_border b]  (undistorts and rectifies one pair with\n"
            "                     the matrices M1 D1 R1 P1 M2 D2 R2 P2 of the OpenCV YAML file f (K1 / K2 for M1 / M2; D of 4, 5 or 8\n"
            "                     entries): writes <left>.rectified.png and <right>.rectified.png at the input's size, a tap outside\n"
            "                     the source reading b (default 0), and prints each image's valid pixels and the call time; with\n"
            "                     --stereo_disparity the pair is rectified first - the flags and the file names are this build's own)\n"
            "       [--rectify_calib f]  (reconstruction run: every image of image_dir, and under --gpu_disparity of right_image_dir,\n"
            "                     is replaced by its rectified version right after it is read; disparities read from\n"
            "                     --disparity_dir are taken to be in rectified coordinates already; single-GPU batched path only)\n"
            "./pose --filter_disparity in.png [the same three flags]  (the filter alone on an 8-bit grey PNG: writes\n"
            "                     <in>.filtered.png and prints the components, the speckles, the removed pixels and the call time;\n"
            "                     at least one of the two filters must be on - the flags and the file name are this build's own)\n"
            "./pose --segment_image image.png [--segment_step s] [--segment_compactness m] [--segment_iterations k] [--segment_min_size n]\n"
            "                     (superpixel labels of one image: grid-seeded k-means of step s (default 16), compactness m (default\n"
            "                     20) and k iterations (default 5), connected components, components below n pixels (default s s / 4)\n"
            "                     merged into their nearest neighbour in colour; writes the labels as <image>.labels.png, 16-bit grey,\n"
            "                     what --segment_labels_dir holds, and prints the centres, components, merged components, labels and\n"
            "                     the call time; an image of more than 65536 labels is refused - the flags and the file name are this\n"
            "                     build's own)\n"
            "       [--use_segment_labels --gpu_segment_labels]  (reconstruction run: every frame's label image comes from the same\n"
            "                     segmentation of its rgb image, after --rectify_calib if given, with the --segment_* flags, instead of\n"
            "                     --segment_labels_dir, which must not be given then)\n"
            "       [--gpu_disparity --right_image_dir d/]  (reconstruction run: every frame's disparity image comes from the same\n"
            "                     matcher on image_dir/<n>.png and d/<n>.png, with the --stereo_* flags, instead of --disparity_dir;\n"
            "                     single-GPU batched path only)\n"
            "       [--feature_poses] [--dist_nearby m] [--range_width n] [--chain_min_matches n] [--chain_max_rms m]\n"
            "       [--chain_ransac_threshold m] [--chain_ransac_iterations n] [--chain_ransac_seed s]\n"
            "       [--refine_poses] [--refine_gn_iterations n] [--refine_cg_iterations n] [--refine_prior_weight w]\n"
            "                     (reconstruction run: every frame's pose from ORB matches against the earlier frames whose recorded\n"
            "                     position lies within --dist_nearby metres (default 2), at most --range_width of them (default 8,\n"
            "                     the most recent); a frame with fewer than --chain_min_matches correspondences (default 30), a\n"
            "                     degenerate fit or an rms above --chain_max_rms is printed as Rejected! and left out of the cloud;\n"
            "                     with --chain_ransac_threshold (metres; absent: off) every frame pair's correspondences first go\n"
            "                     through a three-point RANSAC for a rigid transform (--chain_ransac_iterations hypotheses, default\n"
            "                     256, drawn with --chain_ransac_seed, default 0), the fit uses the inliers only and the frame's line\n"
            "                     gains \"dropped n\", the correspondences the filter took out;\n"
            "                     --dist_nearby, --range_width and the --chain_* flags act under this flag only; shares the extractor call with\n"
            "                     --gpu_keypoints; single-GPU batched path only; the flag is this build's own)\n"
            "                     with --refine_poses every cycle's chain is followed by one joint least-squares refinement of\n"
            "                     the cycle's matched frames over all of its pairs (earlier cycles held; --refine_gn_iterations,\n"
            "                     default 5, Gauss-Newton steps of --refine_cg_iterations, default 32, CG steps; --refine_prior_weight,\n"
            "                     default 0, pulls every free frame's position to its recorded one); one line per cycle reports it\n"
            "       [--multiview_filter] [--mv_neighbors k] [--mv_max_distance m] [--mv_tolerance t] [--mv_min_support n] [--mv_max_violations n]\n"
            "                     (reconstruction run: once a cycle's poses are final and before its frames are accumulated, every\n"
            "                     pixel of every accepted frame is carried into the frame's k nearest accepted frames of the same cycle\n"
            "                     (default 4, none farther than m metres, default: no limit) and stays iff at least n of them (default 1)\n"
            "                     saw the same surface within t disparity levels (default 1) and fewer saw through it than agreed\n"
            "                     (--mv_max_violations n >= 0: at most n saw through it); one line per cycle reports the pixels kept;\n"
            "                     the variance gate has seen the unfiltered image; not available with --gpus N > 1,\n"
            "                     --partitioned_merge, --reference_fanout, --use_segment_labels, --blur_kernel > 1; without the flag the\n"
            "                     --mv_* flags are parsed and ignored; the flags are this build's own)\n"
            "       [--multiview_fuse]\n"
            "                     (reconstruction run: the same step with the same --mv_* flags and neighbours, but every pixel that\n"
            "                     stays is replaced by the mean of its own level and the levels its agreeing neighbours vote for\n"
            "                     (o3dr_multiview_fuse), and the cycle's frames are accumulated as 64-bit float levels; one line per\n"
            "                     cycle reports the pixels kept and the votes; given together with --multiview_filter it means fuse;\n"
            "                     not available where --multiview_filter is not; the flag is this build's own)\n"
            "Without --feature_poses the run uses the recorded MAVLink poses (--only_MAVLink).  The ICP trajectory correction,\n"
            "visualisation and --segment_cloud in a reconstruction run are not part of this build.\n";
}

int Pose::parseCmdArgs(int argc, char** argv)
{
    if (argc == 1) {
        printUsage();
        return -1;
    }
    int n_imgs = 0;
    auto need = [&](int& i) -> const char* {
        if (i + 1 >= argc) throw runtime_error(string("missing value after ") + argv[i]);
        return argv[++i];
    };
    // the one or two file operands of a mode flag (none may begin with "--"; `what` names them): the run is then that tool's
    auto files = [&](int& i, const char* what, string& f0, string* f1 = nullptr) {
        const int n = f1 ? 2 : 1;
        bool ok = i + n < argc;
        for (int k = 1; ok && k <= n; ++k) ok = string(argv[i + k]).rfind("--", 0) != 0;
        if (!ok) throw runtime_error(string("missing argument: ") + argv[i] + " needs " + what);
        f0 = argv[++i];
        if (f1) *f1 = argv[++i];
        run3d_reconstruction = false;
    };
    for (int i = 1; i < argc; ++i) {
        const string a = argv[i];
        if (a == "--help" || a == "/?") { printUsage(); return -1; }
        else if (a == "--downsample") { downsample = true; run3d_reconstruction = false; read_PLY_filename0 = need(i); }
        else if (a == "--align_point_cloud") { files(i, "source.ply and target.ply", read_PLY_filename0, &read_PLY_filename1); align_point_cloud = true; }
        else if (a == "--smooth_surface") { files(i, "file.ply", read_PLY_filename0); smooth_surface = true; }
        else if (a == "--segment_cloud_only") { files(i, "file.ply", read_PLY_filename0); segment_cloud_only = true; }
        else if (a == "--mesh_surface") { files(i, "file.ply", read_PLY_filename0); mesh_surface = true; }
        else if (a == "--mesh_normals") mesh_normals = true;
        else if (a == "--orthophoto") { files(i, "file.ply", read_PLY_filename0); orthophoto = true; }
        else if (a == "--orthophoto_out") orthophoto_out = need(i);
        else if (a == "--ground_filter") { files(i, "file.ply", read_PLY_filename0); ground_filter = true; }
        else if (a == "--ground_max_window") ground_max_window = atoi(need(i));
        else if (a == "--ground_window_base") ground_window_base = atoi(need(i));
        else if (a == "--ground_linear") ground_linear = true;
        else if (a == "--ground_slope") ground_slope = atof(need(i));
        else if (a == "--ground_initial_distance") ground_initial_distance = atof(need(i));
        else if (a == "--ground_max_distance") ground_max_distance = atof(need(i));
        else if (a == "--ground_fill_radius") ground_fill_radius = atoi(need(i));
        else if (a == "--ground_interpolate") ground_interpolate = true;
        else if (a == "--ground_smooth") ground_smooth = atoi(need(i));
        else if (a == "--cluster_cloud") { files(i, "file.ply", read_PLY_filename0); cluster_cloud = true; }
        else if (a == "--cluster_tolerance") { cluster_tolerance = atof(need(i)); cluster_tolerance_set = true; }
        else if (a == "--cluster_min_size") cluster_min_size = atoi(need(i));
        else if (a == "--cluster_max_size") cluster_max_size = atoi(need(i));
        else if (a == "--contours") { files(i, "file.ply", read_PLY_filename0); contours = true; }
        else if (a == "--contour_interval") { contour_interval = atof(need(i)); contour_interval_set = true; }
        else if (a == "--contour_base") contour_base = atof(need(i));
        else if (a == "--contour_surface") contour_surface = need(i);
        else if (a == "--contour_min_segments") contour_min_segments = atoi(need(i));
        else if (a == "--ortho_select") ortho_select = need(i);
        else if (a == "--ortho_fill_radius") ortho_fill_radius = atoi(need(i));
        else if (a == "--ortho_light") {
            if (i + 3 >= argc) throw runtime_error("missing argument: --ortho_light needs lx ly lz");
            for (int k = 0; k < 3; ++k) ortho_light[k] = atof(argv[++i]);
            ortho_light_set = true;
        }
        else if (a == "--sac_distance_threshold") { sac_distance_threshold = atof(need(i)); sac_distance_threshold_set = true; }
        else if (a == "--sac_max_iterations") sac_max_iterations = atoi(need(i));
        else if (a == "--segment_tile_size") segment_tile_size = atof(need(i));
        else if (a == "--sac_seed") sac_seed = strtoull(need(i), nullptr, 0);
        else if (a == "--sac_optimize") sac_optimize = atoi(need(i));
        else if (a == "--mls_polynomial_order") mls_polynomial_order = atoi(need(i));
        else if (a == "--mls_sqr_gauss_param") mls_sqr_gauss_param = atof(need(i));
        else if (a == "--mls_normals") mls_normals = true;
        else if (a == "--icp_max_iterations") icp_max_iterations = atoi(need(i));
        else if (a == "--icp_max_corr_dist") icp_max_corr_dist = atof(need(i));
        else if (a == "--icp_transformation_epsilon") icp_transformation_epsilon = atof(need(i));
        else if (a == "--voxel_size") voxel_size = atof(need(i));
        else if (a == "--min_points_per_voxel") min_points_per_voxel = (unsigned)atoi(need(i));
        else if (a == "--jump_pixels") jump_pixels = atoi(need(i));
        else if (a == "--seq_len") seq_len = atoi(need(i));
        else if (a == "--blur_kernel") blur_kernel = atoi(need(i));
        else if (a == "--log") log_stuff = atoi(need(i)) != 0;
        else if (a == "--dont_downsample") dont_downsample = true;
        else if (a == "--only_MAVLink") only_MAVLink = true;
        else if (a == "--dont_icp") dont_icp = true;
        else if (a == "--reference_fanout") reference_fanout = true;
        else if (a == "--sor") sor = atoi(need(i)) != 0;
        else if (a == "--data_dir") dataFilesPrefix = need(i);
        else if (a == "--image_dir") imagePrefix = need(i);
        else if (a == "--disparity_dir") disparityPrefix = need(i);
        else if (a == "--output_dir") outputPrefix = need(i);
        else if (a == "--keypoints_dir") keypointsPrefix = need(i);
        else if (a == "--calib_file") calib_file = need(i);
        else if (a == "--device") device_id = atoi(need(i));
        else if (a == "--gpus") n_gpus = atoi(need(i));
        else if (a == "--partitioned_merge") partitioned_merge = true;
        else if (a == "--search_radius") { search_radius = atof(need(i)); search_radius_set = true; }  // --smooth_surface, --mesh_surface
        else if (a == "--dist_nearby") dist_nearby = atof(need(i));  // (both act with --feature_poses only)
        else if (a == "--range_width") range_width = atoi(need(i));
        else if (a == "--feature_poses") feature_poses = true;
        else if (a == "--chain_min_matches") chain_min_matches = atoi(need(i));
        else if (a == "--chain_max_rms") chain_max_rms = atof(need(i));
        else if (a == "--chain_ransac_threshold") { chain_ransac_threshold = atof(need(i)); chain_ransac = true; }
        else if (a == "--chain_ransac_iterations") chain_ransac_iterations = atoi(need(i));
        else if (a == "--chain_ransac_seed") chain_ransac_seed = strtoull(need(i), nullptr, 0);
        else if (a == "--refine_poses") refine_poses = true;
        else if (a == "--refine_gn_iterations") refine_gn_iterations = atoi(need(i));
        else if (a == "--refine_cg_iterations") refine_cg_iterations = atoi(need(i));
        else if (a == "--refine_prior_weight") refine_prior_weight = atof(need(i));
        else if (a == "--preview") preview = true;
        else if (a == "--use_segment_labels") use_segment_labels = true;
        else if (a == "--segment_labels_dir") { segmentLabelsPrefix = need(i); segment_labels_dir_set = true; }
        else if (a == "--gpu_segment_labels") gpu_segment_labels = true;
        else if (a == "--segment_image") files(i, "image.png", segment_image_png);
        else if (a == "--segment_step") segment_step = atoi(need(i));
        else if (a == "--segment_compactness") segment_compactness = atoi(need(i));
        else if (a == "--segment_iterations") segment_iterations = atoi(need(i));
        else if (a == "--segment_min_size") segment_min_size = atoi(need(i));
        else if (a == "--plane_min_pixels") plane_min_pixels = atoi(need(i));
        else if (a == "--plane_max_mse") plane_max_mse = atof(need(i));
        else if (a == "--find_features") files(i, "image.png", find_features_png);
        else if (a == "--stereo_disparity") files(i, "left.png and right.png", stereo_left_png, &stereo_right_png);
        else if (a == "--gpu_disparity") gpu_disparity = true;
        else if (a == "--right_image_dir") rightImagePrefix = need(i);
        else if (a == "--stereo_n_disparities") stereo_n_disparities = atoi(need(i));
        else if (a == "--stereo_min_disparity") stereo_min_disparity = atoi(need(i));
        else if (a == "--stereo_p1") stereo_p1 = atoi(need(i));
        else if (a == "--stereo_p2") stereo_p2 = atoi(need(i));
        else if (a == "--stereo_paths") stereo_paths = atoi(need(i));
        else if (a == "--stereo_uniqueness") stereo_uniqueness = atoi(need(i));
        else if (a == "--stereo_lr_max_diff") stereo_lr_max_diff = atoi(need(i));
        else if (a == "--stereo_median") stereo_median = atoi(need(i));
        else if (a == "--stereo_speckle_size") stereo_speckle_size = atoi(need(i));
        else if (a == "--stereo_speckle_diff") stereo_speckle_diff = atoi(need(i));
        else if (a == "--filter_disparity") files(i, "in.png", filter_disparity_png);
        else if (a == "--rectify_pair") files(i, "left.png and right.png", rectify_left_png, &rectify_right_png);
        else if (a == "--rectify_calib") rectify_calib = need(i);
        else if (a == "--rectify_border") rectify_border = atoi(need(i));
        else if (a == "--gpu_keypoints") gpu_keypoints = true;
        else if (a == "--orb_n_features") orb_n_features = atoi(need(i));
        else if (a == "--orb_levels") orb_levels = atoi(need(i));
        else if (a == "--orb_scale") orb_scale = (float)atof(need(i));
        else if (a == "--orb_fast_threshold") orb_fast_threshold = atoi(need(i));
        else if (a == "--multiview_filter") multiview_filter = true;
        else if (a == "--multiview_fuse") multiview_fuse = true;
        else if (a == "--mv_neighbors") mv_neighbors = atoi(need(i));
        else if (a == "--mv_max_distance") mv_max_distance = atof(need(i));
        else if (a == "--mv_tolerance") mv_tolerance = atof(need(i));
        else if (a == "--mv_min_support") mv_min_support = atoi(need(i));
        else if (a == "--mv_max_violations") mv_max_violations = atoi(need(i));
        else if (a == "--print_label_png") { print_label_png = need(i); run3d_reconstruction = false; }
        else if (a == "--segment_cloud" || a == "--displayUAVPositions" ||
                 a == "--test_bad_data_rejection")
            cout << a << ": outside the hot path, ignored in this build" << endl;
        else if (a.rfind("--", 0) == 0) throw runtime_error("unknown flag " + a);
        else {  // positional image numbers (:247-256)
            if (first_img_num == -1) first_img_num = atoi(argv[i]); else last_img_num = atoi(argv[i]);
            ++n_imgs;
        }
    }
    // A feature of the single-GPU batched path says so on the other paths instead of dropping its flag: the first refusal that
    // applies, --gpus N and --partitioned_merge in one message (combined) or in one each
    auto batched_path_only = [&](const string& flag, bool combined) {
        const string head = flag + " is not available with ";
        if (combined && (n_gpus > 1 || partitioned_merge)) throw runtime_error(head + "--gpus N > 1 / --partitioned_merge");
        if (n_gpus > 1) throw runtime_error(head + "--gpus N > 1");
        if (partitioned_merge) throw runtime_error(head + "--partitioned_merge");
        if (reference_fanout) throw runtime_error(head + "--reference_fanout");
    };
    if (run3d_reconstruction && use_segment_labels) {
        batched_path_only("--use_segment_labels", true);
        if (blur_kernel > 1) throw runtime_error("--use_segment_labels cannot be combined with --blur_kernel > 1 (cv::bilateralFilter rejects CV_64F)");
    }
    if (run3d_reconstruction && (multiview_filter || multiview_fuse)) {
        // the filter sits between the cycle's poses and the batched accumulate call, the fusion where the filter does (it
        // hands that call float64 images of its own); given together, the two flags mean fuse
        const string flag = multiview_fuse ? "--multiview_fuse" : "--multiview_filter";
        batched_path_only(flag, false);
        if (use_segment_labels) throw runtime_error(flag + " is not available with --use_segment_labels (its images are CV_64F fits)");
        if (blur_kernel > 1)
            throw runtime_error(flag + " is not available with --blur_kernel > 1 (the blur would run on the " + (multiview_fuse ? "fused" : "filtered") + " image)");
        if (multiview_fuse) multiview_filter = false;
    }
    if (run3d_reconstruction && gpu_segment_labels) {
        if (!use_segment_labels) throw runtime_error("--gpu_segment_labels makes the labels of --use_segment_labels: give both");
        if (segment_labels_dir_set) throw runtime_error("--gpu_segment_labels cannot be combined with --segment_labels_dir");
    }
    if (!segment_image_png.empty() && !ifstream(segment_image_png)) throw runtime_error("could not read " + segment_image_png);
    if (orthophoto || (run3d_reconstruction && !orthophoto_out.empty())) {
        if (run3d_reconstruction) {
            batched_path_only("--orthophoto_out", false);
        } else if (!ifstream(read_PLY_filename0)) {
            throw runtime_error("could not read " + read_PLY_filename0);
        }
        if (ortho_select != "first" && ortho_select != "top" && ortho_select != "bottom")
            throw runtime_error("--ortho_select must be first, top or bottom");
        if (ortho_fill_radius < 0 || ortho_fill_radius > O3DR_RASTER_MAX_FILL_RADIUS) throw runtime_error("--ortho_fill_radius must be in 0..32");
        const double ln = sqrt((ortho_light[0] * ortho_light[0] + ortho_light[1] * ortho_light[1]) + ortho_light[2] * ortho_light[2]);
        if (ortho_light_set && !(isfinite(ln) && ln > 0.0)) throw runtime_error("--ortho_light must be a finite vector that is not zero");
    }
    if (ground_filter) {
        if (!ifstream(read_PLY_filename0)) throw runtime_error("could not read " + read_PLY_filename0);
        if (ground_max_window < 1 || ground_max_window > O3DR_GROUND_MAX_WINDOW_RADIUS) throw runtime_error("--ground_max_window must be in 1..128");
        if (ground_window_base < (ground_linear ? 1 : 2))
            throw runtime_error("--ground_window_base must be >= 2, or >= 1 with --ground_linear");
        if (ground_linear && ground_window_base > ground_max_window)
            throw runtime_error("--ground_window_base must not exceed --ground_max_window with --ground_linear (no window fits)");
        if (!(isfinite(ground_slope) && ground_slope >= 0.0)) throw runtime_error("--ground_slope must be finite and >= 0");
        if (!(isfinite(ground_initial_distance) && ground_initial_distance >= 0.0))
            throw runtime_error("--ground_initial_distance must be finite and >= 0");
        if (!(isfinite(ground_max_distance) && ground_max_distance >= 0.0)) throw runtime_error("--ground_max_distance must be finite and >= 0");
        if (ground_fill_radius < 0 || ground_fill_radius > O3DR_RASTER_MAX_FILL_RADIUS) throw runtime_error("--ground_fill_radius must be in 0..32");
        if (ground_interpolate && ground_fill_radius != 0) throw runtime_error("--ground_interpolate needs --ground_fill_radius 0 (the interpolation is the fill)");
        if (ground_interpolate && (ground_smooth < 0 || ground_smooth > O3DR_INTERPOLATE_MAX_SMOOTH)) throw runtime_error("--ground_smooth must be in 0..8");
    }
    if (cluster_cloud) {
        if (!ifstream(read_PLY_filename0)) throw runtime_error("could not read " + read_PLY_filename0);
        if (!cluster_tolerance_set) throw runtime_error("--cluster_cloud needs --cluster_tolerance t (metres)");
        if (!(isfinite(cluster_tolerance) && cluster_tolerance > 0.0)) throw runtime_error("--cluster_tolerance must be finite and > 0");
        if (cluster_min_size < 1) throw runtime_error("--cluster_min_size must be >= 1");
        if (cluster_max_size < cluster_min_size) throw runtime_error("--cluster_max_size must be >= --cluster_min_size");
    }
    if (contours) {
        if (!ifstream(read_PLY_filename0)) throw runtime_error("could not read " + read_PLY_filename0);
        if (!contour_interval_set) throw runtime_error("--contours needs --contour_interval m (metres)");
        if (!(isfinite(contour_interval) && contour_interval > 0.0)) throw runtime_error("--contour_interval must be finite and > 0");
        if (!isfinite(contour_base)) throw runtime_error("--contour_base must be finite");
        if (contour_surface != "dtm" && contour_surface != "dsm") throw runtime_error("--contour_surface must be dtm or dsm");
        if (contour_min_segments < 1) throw runtime_error("--contour_min_segments must be >= 1");
    }
    if (run3d_reconstruction && gpu_keypoints) batched_path_only("--gpu_keypoints", true);
    if (run3d_reconstruction && gpu_disparity) {
        batched_path_only("--gpu_disparity", true);
        if (use_segment_labels) throw runtime_error("--gpu_disparity is not available with --use_segment_labels");
        if (rightImagePrefix.empty()) throw runtime_error("--gpu_disparity needs --right_image_dir d/");
    }
    if (!rectify_left_png.empty() && rectify_calib.empty()) throw runtime_error("--rectify_pair needs --rectify_calib f");
    if (!rectify_calib.empty()) {
        if (run3d_reconstruction) batched_path_only("--rectify_calib", true);
        if (rectify_border < 0 || rectify_border > 255) throw runtime_error("--rectify_border must be in 0..255");
        readRectifyCalib();
    }
    if (!filter_disparity_png.empty()) {
        if (!disparity_filter_on())
            throw runtime_error("--filter_disparity needs a filter: give --stereo_median 3|5 and / or --stereo_speckle_size n");
        if (!ifstream(filter_disparity_png)) throw runtime_error("could not read " + filter_disparity_png);
    }
    if (refine_poses && !feature_poses) throw runtime_error("--refine_poses refines the poses of --feature_poses: give both");
    if (run3d_reconstruction && feature_poses) batched_path_only("--feature_poses", true);
    if (run3d_reconstruction) {
        if (n_imgs == 0) throw runtime_error("first and last image number are required");
        if (last_img_num < first_img_num) last_img_num = first_img_num;
        readPoseFile();
        n_imgs = last_img_num - first_img_num + 1;  // :300-303
        rawImageDataVec = vector<RawImageData>((size_t)n_imgs);
        for (int i = 0; i < n_imgs; ++i) rawImageDataVec[i].img_num = first_img_num + i;
    }
    return 0;
}

// pose.cpp:46-112: pcl::IterativeClosestPoint of source onto target, here o3dr_icp_align (contract: include/o3dr.h).  The
// result is printed and the source, moved by fp32(T) through transformPtCloud, is written as aligned_<source> next to it.
void Pose::run_align_point_cloud()
{
    PointCloud::Ptr src = read_PLY_File(read_PLY_filename0);
    PointCloud::Ptr tgt = read_PLY_File(read_PLY_filename1);
    o3dr_icp_params prm;
    o3dr_icp_default_params(&prm);
    prm.max_iterations = icp_max_iterations;
    prm.max_correspondence_distance = icp_max_corr_dist;
    prm.transformation_epsilon = icp_transformation_epsilon;
    o3dr_icp_result res;
    chk(o3dr_icp_align(ctx_for_this_thread(), src->points.data(), (int64_t)src->points.size(), tgt->points.data(),
                       (int64_t)tgt->points.size(), nullptr, &prm, &res, O3DR_MEM_HOST),
        "o3dr_icp_align");
    char line[256];
    cout << "ICP transformation (source -> target):" << endl;
    for (int r = 0; r < 4; ++r) {
        snprintf(line, sizeof line, "%.17g %.17g %.17g %.17g", res.T[4 * r], res.T[4 * r + 1], res.T[4 * r + 2], res.T[4 * r + 3]);
        cout << line << endl;
    }
    snprintf(line, sizeof line, "fitness %.17g", res.fitness);
    cout << line << endl;
    cout << "correspondences " << res.n_correspondences << endl;
    cout << "iterations " << res.iterations << endl;
    cout << "reason " << (res.reason >= 0 && res.reason < 5 ? kIcpReasonName[res.reason] : "?") << endl;
    Matrix4 Tf;
    for (int k = 0; k < 16; ++k) Tf[k] = (float)res.T[k];
    PointCloud::Ptr aligned(new PointCloud());
    if (!src->points.empty()) transformPtCloud(src, aligned, Tf);
    string out = next_to(read_PLY_filename0, "aligned_");
    save_pt_cloud_to_PLY_File(aligned, out);
}

// pose.cpp:27-112 --smooth_surface: pcl::MovingLeastSquares over one PLY, here o3dr_mls_smooth (contract: include/o3dr.h).
// The points with a fit (MLS_POLY or MLS_PLANE) are written in input order as smoothed_<file> next to it, with
// --mls_normals in PointXYZRGBNormal's layout.
void Pose::run_smooth_surface()
{
    if (!search_radius_set) throw runtime_error("missing argument: --smooth_surface needs --search_radius r");
    PointCloud::Ptr cloud = read_PLY_File(read_PLY_filename0);
    const int64_t n = (int64_t)cloud->points.size();
    o3dr_mls_params prm;
    o3dr_mls_default_params(&prm);
    prm.search_radius = search_radius;
    prm.polynomial_order = mls_polynomial_order;
    prm.sqr_gauss_param = mls_sqr_gauss_param;
    vector<PointXYZRGB> out((size_t)n);
    vector<float> nrm(mls_normals ? (size_t)n * 4 : 0);
    vector<uint8_t> fit((size_t)n);
    o3dr_mls_result res;
    o3dr_ctx* c = ctx_for_this_thread();
    const auto t0 = chrono::steady_clock::now();
    chk(o3dr_mls_smooth(c, cloud->points.data(), n, &prm, out.data(), mls_normals ? nrm.data() : nullptr, nullptr, fit.data(), &res,
                        O3DR_MEM_HOST),
        "o3dr_mls_smooth");
    const double ms = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
    PointCloud::Ptr kept(new PointCloud());
    vector<float> kept_nrm;
    for (int64_t i = 0; i < n; ++i) {
        if (fit[(size_t)i] == O3DR_MLS_NONE) continue;
        kept->points.push_back(out[(size_t)i]);
        if (mls_normals) kept_nrm.insert(kept_nrm.end(), nrm.begin() + 4 * i, nrm.begin() + 4 * i + 4);
    }
    cout << "points in " << n << endl;
    cout << "fitted " << res.n_poly + res.n_plane << " (poly " << res.n_poly << ", plane " << res.n_plane << ")" << endl;
    cout << "dropped " << res.n_none << endl;
    cout << "max neighbors " << res.max_neighbors << endl;
    char line[64];
    snprintf(line, sizeof line, "mls time %.3f ms", ms);
    cout << line << endl;
    const string outp = next_to(read_PLY_filename0, "smoothed_");
    if (!save_ply_binary(outp, *kept, mls_normals ? &kept_nrm : nullptr)) throw runtime_error("could not write " + outp);
    cerr << "Saved Point Cloud with " << kept->points.size() << " data points to " << outp << endl;
}

// pose_functions.cpp:2094-2249 segmentCloud, its SACSegmentation (plane, RANSAC, optimizeCoefficients) and ProjectInliers
// here o3dr_segment_plane over one PLY (contract: include/o3dr.h).  The inliers, projected onto their tile's plane, go to
// ground_<file> and the other points to nonground_<file>, both in input order, next to the source.
void Pose::run_segment_cloud()
{
    if (!sac_distance_threshold_set) throw runtime_error("missing argument: --segment_cloud_only needs --sac_distance_threshold t");
    PointCloud::Ptr cloud = read_PLY_File(read_PLY_filename0);
    const int64_t n = (int64_t)cloud->points.size();
    o3dr_plane_params prm;
    o3dr_plane_default_params(&prm);
    prm.distance_threshold = sac_distance_threshold;
    prm.max_iterations = sac_max_iterations;
    prm.tile_size = segment_tile_size;
    prm.seed = sac_seed;
    prm.optimize = sac_optimize;
    vector<uint8_t> inl((size_t)n);
    vector<PointXYZRGB> proj((size_t)n);
    vector<o3dr_plane_tile> tiles(segment_tile_size > 0.0 ? 256 : 1);
    int64_t n_tiles = 0;
    o3dr_ctx* c = ctx_for_this_thread();
    const auto t0 = chrono::steady_clock::now();
    int rc = o3dr_segment_plane(c, cloud->points.data(), n, &prm, inl.data(), nullptr, proj.data(), tiles.data(),
                                (int64_t)tiles.size(), &n_tiles, O3DR_MEM_HOST);
    if (rc == O3DR_ERR_CAPACITY) {
        tiles.resize((size_t)n_tiles);
        rc = o3dr_segment_plane(c, cloud->points.data(), n, &prm, inl.data(), nullptr, proj.data(), tiles.data(),
                                (int64_t)tiles.size(), &n_tiles, O3DR_MEM_HOST);
    }
    chk(rc, "o3dr_segment_plane");
    const double ms = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
    PointCloud::Ptr ground(new PointCloud()), rest(new PointCloud());
    for (int64_t i = 0; i < n; ++i) {
        if (inl[(size_t)i]) ground->points.push_back(proj[(size_t)i]);
        else rest->points.push_back(cloud->points[(size_t)i]);
    }
    cout << "points in " << n << endl;
    cout << "tiles " << n_tiles << endl;
    cout << "inliers " << ground->points.size() << endl;
    char line[256];
    for (int64_t k = 0; k < n_tiles && k < 10; ++k) {
        const o3dr_plane_tile& r = tiles[(size_t)k];
        snprintf(line, sizeof line, "tile %lld (%d, %d): points %u inliers %u status %d refined %d coeff %.9g %.9g %.9g %.9g", (long long)k,
                 r.ix, r.iy, r.n_points, r.n_inliers, r.status, r.refined, r.coeff[0], r.coeff[1], r.coeff[2], r.coeff[3]);
        cout << line << endl;
    }
    if (n_tiles > 10) cout << "... and " << n_tiles - 10 << " more tiles" << endl;
    snprintf(line, sizeof line, "segment time %.3f ms", ms);
    cout << line << endl;
    for (const auto& out : {make_pair("ground_", ground), make_pair("nonground_", rest)}) {
        const string path = next_to(read_PLY_filename0, out.first);
        if (!save_ply_binary(path, *out.second)) throw runtime_error("could not write " + path);
        cerr << "Saved Point Cloud with " << out.second->points.size() << " data points to " << path << endl;
    }
}

// pose.cpp:27-112 --mesh_surface: pcl::GreedyProjectionTriangulation over one PLY, here o3dr_mesh_surface's height-field
// triangulation of the occupied XY cells of --voxel_size (contract: include/o3dr.h; the differences from GP3 are in
// INTEGRATION.md).  Every point is written in input order, then the triangles, as mesh_<file> next to the source.
void Pose::run_mesh_surface()
{
    if (!search_radius_set) throw runtime_error("missing argument: --mesh_surface needs --search_radius L");
    PointCloud::Ptr cloud = read_PLY_File(read_PLY_filename0);
    const int64_t n = (int64_t)cloud->points.size();
    o3dr_mesh_params prm;
    o3dr_mesh_default_params(&prm);
    prm.cell_size = voxel_size;
    prm.max_edge_length = search_radius;
    vector<int32_t> tris((size_t)(2 * n) * 3);  // at most 2 triangles per vertex
    vector<float> nrm(mesh_normals ? (size_t)n * 3 : 0);
    int64_t n_tris = 0;
    o3dr_mesh_result res;
    o3dr_ctx* c = ctx_for_this_thread();
    const auto t0 = chrono::steady_clock::now();
    chk(o3dr_mesh_surface(c, cloud->points.data(), n, &prm, tris.data(), 2 * n, &n_tris, mesh_normals ? nrm.data() : nullptr, &res,
                          O3DR_MEM_HOST),
        "o3dr_mesh_surface");
    const double ms = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
    tris.resize((size_t)n_tris * 3);
    cout << "points in " << n << endl;
    cout << "vertices " << res.n_vertices << " (shadowed points " << res.n_shadowed << ")" << endl;
    cout << "triangles " << res.n_triangles << " (full quads " << res.n_quads_full << ")" << endl;
    cout << "rejected orientation " << res.n_rejected_orientation << ", length " << res.n_rejected_length << endl;
    char line[64];
    snprintf(line, sizeof line, "mesh time %.3f ms", ms);
    cout << line << endl;
    const string outp = next_to(read_PLY_filename0, "mesh_");
    if (!save_ply_mesh(outp, *cloud, tris, mesh_normals ? &nrm : nullptr)) throw runtime_error("could not write " + outp);
    cerr << "Saved mesh with " << n << " vertices and " << n_tris << " faces to " << outp << endl;
}

// --orthophoto: the map of one PLY as images (o3dr_rasterize_map; contract: include/o3dr.h "map raster"), written as
// ortho_<file>.png, height_<file>.png and, with --ortho_light, shade_<file>.png next to the source.
void Pose::run_orthophoto()
{
    PointCloud::Ptr cloud = read_PLY_File(read_PLY_filename0);
    const string& src = read_PLY_filename0;
    write_map_rasters(ctx_for_this_thread(), *cloud, next_to(src, "ortho_", ".png"), next_to(src, "height_", ".png"), next_to(src, "shade_", ".png"));
}

void Pose::write_map_rasters(o3dr_ctx* c, const PointCloud& cloud, const string& ortho_path, const string& height_path,
                             const string& shade_path)
{
    const int64_t n = (int64_t)cloud.points.size();
    o3dr_raster_params prm;
    o3dr_raster_default_params(&prm);
    prm.cell_size = voxel_size;
    prm.select = ortho_select == "top" ? O3DR_RASTER_TOP : ortho_select == "bottom" ? O3DR_RASTER_BOTTOM : O3DR_RASTER_FIRST;
    prm.fill_radius = ortho_fill_radius;
    prm.use_light = ortho_light_set ? 1 : 0;
    for (int k = 0; k < 3 && ortho_light_set; ++k) prm.light[k] = ortho_light[k];
    const auto t0 = chrono::steady_clock::now();
    chk(o3dr_raster_extent(c, cloud.points.data(), n, voxel_size, &prm.cx0, &prm.cy0, &prm.width, &prm.height, O3DR_MEM_HOST),
        "o3dr_raster_extent");
    const int W = prm.width, H = prm.height;
    const size_t cells = (size_t)W * (size_t)H;
    vector<float> height(cells);
    vector<uint8_t> color(cells * 3), shade(ortho_light_set ? cells : 0);
    o3dr_raster_outputs out = {height.data(), color.data(), ortho_light_set ? shade.data() : nullptr, nullptr, nullptr};
    o3dr_raster_result res;
    chk(o3dr_rasterize_map(c, cloud.points.data(), n, &prm, &out, &res, O3DR_MEM_HOST), "o3dr_rasterize_map");
    const double ms = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
    // the heights as 16-bit grey: 0 = no data, else 1 + min(65534, floor((z - z_min) / step)), fp64
    const double step = max(((double)res.z_max - (double)res.z_min) / 65534.0, ldexp(1.0, -15));
    vector<uint16_t> h16(cells);
    vector<uint8_t> color_up(cells * 3), shade_up(shade.size());
    for (int r = 0; r < H; ++r) {  // rows in descending cy: north up, not mirrored
        const size_t src = (size_t)(H - 1 - r) * W, dst = (size_t)r * W;
        for (int x = 0; x < W; ++x) {
            const float z = height[src + x];
            h16[dst + x] = z != z ? 0 : (uint16_t)(1 + (int)min(65534.0, floor(((double)z - (double)res.z_min) / step)));
        }
        memcpy(&color_up[dst * 3], &color[src * 3], (size_t)W * 3);
        if (ortho_light_set) memcpy(&shade_up[dst], &shade[src], (size_t)W);
    }
    char line[256];
    cout << "points in " << n << " (outside the box " << res.n_outside << ")" << endl;
    cout << "box cx0 " << res.cx0 << " cy0 " << res.cy0 << " width " << res.width << " height " << res.height << endl;
    cout << "cells occupied " << res.n_occupied << " (shadowed points " << res.n_shadowed << "), filled " << res.n_filled << ", empty "
         << res.n_empty << endl;
    snprintf(line, sizeof line, "z_min %.9g z_max %.9g step %.17g", (double)res.z_min, (double)res.z_max, step);
    cout << line << endl;
    snprintf(line, sizeof line, "raster time %.3f ms", ms);
    cout << line << endl;
    if (!write_png_bgr8(ortho_path, color_up.data(), H, W)) throw runtime_error("could not write " + ortho_path);
    if (!write_png_grey16(height_path, h16.data(), H, W)) throw runtime_error("could not write " + height_path);
    if (ortho_light_set && !write_png_grey8(shade_path, shade_up.data(), H, W)) throw runtime_error("could not write " + shade_path);
    cerr << "Saved " << W << " x " << H << " map rasters to " << ortho_path << ", " << height_path
         << (ortho_light_set ? ", " + shade_path : string()) << endl;
}

// --ground_filter: the ground points, the others and the terrain model of one PLY (o3dr_ground_filter; contract:
// include/o3dr_terrain.h "ground filter"), written as terrain_<file>, objects_<file> and dtm_<file>.png next to the source.
void Pose::run_ground_filter()
{
    PointCloud::Ptr cloud = read_PLY_File(read_PLY_filename0);
    const int64_t n = (int64_t)cloud->points.size();
    o3dr_ground_params prm;
    o3dr_ground_default_params(&prm);
    prm.cell_size = voxel_size;
    prm.max_window_radius = ground_max_window, prm.window_base = ground_window_base, prm.exponential = ground_linear ? 0 : 1;
    prm.slope = ground_slope, prm.initial_distance = ground_initial_distance, prm.max_distance = ground_max_distance;
    prm.fill_radius = ground_fill_radius;
    int32_t radii[16], n_iter = 0;
    float thr[16];
    chk(o3dr_ground_schedule(&prm, radii, thr, &n_iter), "o3dr_ground_schedule");
    o3dr_ctx* c = ctx_for_this_thread();
    const auto t0 = chrono::steady_clock::now();
    chk(o3dr_raster_extent(c, cloud->points.data(), n, voxel_size, &prm.cx0, &prm.cy0, &prm.width, &prm.height, O3DR_MEM_HOST),
        "o3dr_raster_extent");
    const int W = prm.width, H = prm.height;
    const size_t cells = (size_t)W * (size_t)H;
    vector<uint8_t> ground((size_t)n);
    vector<float> dtm(cells);
    o3dr_ground_outputs out = {ground.data(), nullptr, dtm.data(), nullptr};
    o3dr_ground_result res;
    chk(o3dr_ground_filter(c, cloud->points.data(), n, &prm, &out, &res, O3DR_MEM_HOST), "o3dr_ground_filter");
    o3dr_interpolate_result dem;
    if (ground_interpolate) {  // the DTM from the ground cells alone, at any distance
        o3dr_interpolate_params ip;
        o3dr_interpolate_default_params(&ip);
        ip.width = W, ip.height = H, ip.smooth = ground_smooth;
        vector<float> filled(cells);
        o3dr_interpolate_outputs io = {filled.data(), nullptr};
        chk(o3dr_raster_interpolate(c, dtm.data(), &ip, &io, &dem, O3DR_MEM_HOST), "o3dr_raster_interpolate");
        dtm.swap(filled);
    }
    const double ms = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
    PointCloud::Ptr terrain(new PointCloud()), objects(new PointCloud());
    for (int64_t i = 0; i < n; ++i) (ground[(size_t)i] ? terrain : objects)->points.push_back(cloud->points[(size_t)i]);
    // the DTM as 16-bit grey, the height PNG's encoding from the DTM's own z range (-0.0f taken as 0.0f)
    float z_min = NAN, z_max = NAN;
    for (float z : dtm)
        if (z == z) {
            z = z == 0.f ? 0.f : z;
            z_min = z_min == z_min ? min(z_min, z) : z, z_max = z_max == z_max ? max(z_max, z) : z;
        }
    const double step = max(((double)z_max - (double)z_min) / 65534.0, ldexp(1.0, -15));
    vector<uint16_t> d16(cells);
    for (int r = 0; r < H; ++r) {  // rows in descending cy: north up, not mirrored
        const size_t src = (size_t)(H - 1 - r) * W, dst = (size_t)r * W;
        for (int x = 0; x < W; ++x) {
            const float z = dtm[src + x];
            d16[dst + x] = z != z ? 0 : (uint16_t)(1 + (int)min(65534.0, floor(((double)z - (double)z_min) / step)));
        }
    }
    char line[256];
    cout << "points in " << n << " (outside the box " << res.n_outside << ")" << endl;
    cout << "box cx0 " << res.cx0 << " cy0 " << res.cy0 << " width " << res.width << " height " << res.height << endl;
    for (int k = 0; k < n_iter; ++k) {
        snprintf(line, sizeof line, "iteration %d radius %d threshold %.9g removed cells %lld", k, radii[k], (double)thr[k],
                 (long long)res.n_removed[k]);
        cout << line << endl;
    }
    cout << "cells occupied " << res.n_occupied << ", ground " << res.n_ground_cells << ", dtm filled " << res.n_dtm_filled << ", dtm empty "
         << res.n_dtm_empty << endl;
    cout << "ground points " << res.n_ground_points << ", object points " << n - res.n_ground_points << endl;
    if (ground_interpolate)
        cout << "dtm interpolated: " << dem.n_data << " data cells, " << dem.n_filled << " filled, " << dem.n_levels << " levels" << endl;
    snprintf(line, sizeof line, "dtm z_min %.9g z_max %.9g step %.17g", (double)z_min, (double)z_max, step);
    cout << line << endl;
    snprintf(line, sizeof line, "ground filter time %.3f ms", ms);
    cout << line << endl;
    for (const auto& o : {make_pair("terrain_", terrain), make_pair("objects_", objects)}) {
        const string path = next_to(read_PLY_filename0, o.first);
        if (!save_ply_binary(path, *o.second)) throw runtime_error("could not write " + path);
        cerr << "Saved Point Cloud with " << o.second->points.size() << " data points to " << path << endl;
    }
    const string dtm_path = next_to(read_PLY_filename0, "dtm_", ".png");
    if (!write_png_grey16(dtm_path, d16.data(), H, W)) throw runtime_error("could not write " + dtm_path);
    cerr << "Saved " << W << " x " << H << " terrain model to " << dtm_path << endl;
}

// --cluster_cloud: the objects of one PLY (o3dr_cluster_euclidean; contract: include/o3dr_objects.h), written as
// clusters_<file>, unclustered_<file> and clusters_<file>.txt next to the source.
void Pose::run_cluster_cloud()
{
    PointCloud::Ptr cloud = read_PLY_File(read_PLY_filename0);
    const int64_t n = (int64_t)cloud->points.size();
    o3dr_cluster_params prm;
    o3dr_cluster_default_params(&prm);
    prm.tolerance = cluster_tolerance, prm.min_size = cluster_min_size, prm.max_size = cluster_max_size;
    vector<int32_t> label((size_t)n), indices((size_t)n);
    vector<o3dr_cluster> rec((size_t)(n / cluster_min_size));  // no more clusters fit in n points
    o3dr_cluster_outputs out = {label.data(), nullptr, nullptr, indices.data()};
    o3dr_cluster_result res;
    int64_t K = 0;
    o3dr_ctx* c = ctx_for_this_thread();
    const auto t0 = chrono::steady_clock::now();
    chk(o3dr_cluster_euclidean(c, cloud->points.data(), n, &prm, &out, rec.empty() ? nullptr : rec.data(), (int64_t)rec.size(), &K, &res,
                               O3DR_MEM_HOST),
        "o3dr_cluster_euclidean");
    const double ms = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
    // the clustered points in indices order, a colour per cluster number (a hash: neighbours in number differ); the others
    PointCloud::Ptr clustered(new PointCloud()), rest(new PointCloud());
    for (int64_t k = 0; k < K; ++k) {
        const uint32_t h = (uint32_t)(k + 1) * 2654435761u;
        const uint32_t rgba = 0xff000000u | (h >> 8) | 0x00404040u;
        for (int32_t j = rec[(size_t)k].begin; j < rec[(size_t)k].begin + rec[(size_t)k].size; ++j) {
            auto p = cloud->points[(size_t)indices[(size_t)j]];
            p.rgba = rgba;
            clustered->points.push_back(p);
        }
    }
    for (int64_t i = 0; i < n; ++i)
        if (label[(size_t)i] < 0) rest->points.push_back(cloud->points[(size_t)i]);
    char line[512];
    const string txt_path = next_to(read_PLY_filename0, "clusters_", ".txt");
    ofstream txt(txt_path);
    cout << "points in " << n << ", linked pairs " << res.n_pairs << endl;
    cout << "components " << res.n_components << " (largest " << res.largest << "), clusters " << res.n_clusters << ", too small " << res.n_too_small
         << ", too large " << res.n_too_large << endl;
    cout << "clustered points " << res.n_clustered_points << ", other points " << res.n_rejected_points << endl;
    for (int64_t k = 0; k < K; ++k) {
        const o3dr_cluster& r = rec[(size_t)k];
        snprintf(line, sizeof line, "%lld %d %d %.9g %.9g %.9g %.9g %.9g %.9g %.17g %.17g %.17g", (long long)k, r.first, r.size, (double)r.lo[0],
                 (double)r.lo[1], (double)r.lo[2], (double)r.hi[0], (double)r.hi[1], (double)r.hi[2], r.centroid[0], r.centroid[1], r.centroid[2]);
        txt << line << "\n";
        if (k < 10) cout << "cluster " << line << endl;
    }
    txt.close();
    if (!txt) throw runtime_error("could not write " + txt_path);
    snprintf(line, sizeof line, "cluster time %.3f ms", ms);
    cout << line << endl;
    for (const auto& o : {make_pair("clusters_", clustered), make_pair("unclustered_", rest)}) {
        const string path = next_to(read_PLY_filename0, o.first);
        if (!save_ply_binary(path, *o.second)) throw runtime_error("could not write " + path);
        cerr << "Saved Point Cloud with " << o.second->points.size() << " data points to " << path << endl;
    }
    cerr << "Saved " << K << " cluster records to " << txt_path << endl;
}

// --contours: the contour lines of one PLY's terrain model (o3dr_raster_contours; contract: include/o3dr_contour.h), written
// as contours_<file>.geojson next to the source.  dtm: the ground filter's DTM at its defaults, interpolated
// (o3dr_ground_filter, o3dr_raster_interpolate); dsm: the raster of every cell's highest point (o3dr_rasterize_map).
void Pose::run_contours()
{
    PointCloud::Ptr cloud = read_PLY_File(read_PLY_filename0);
    const int64_t n = (int64_t)cloud->points.size();
    o3dr_ctx* c = ctx_for_this_thread();
    o3dr_contour_params prm;
    o3dr_contour_default_params(&prm);
    prm.interval = contour_interval, prm.base = contour_base, prm.cell_size = voxel_size;
    chk(o3dr_raster_extent(c, cloud->points.data(), n, voxel_size, &prm.cx0, &prm.cy0, &prm.width, &prm.height, O3DR_MEM_HOST),
        "o3dr_raster_extent");
    const size_t cells = (size_t)prm.width * (size_t)prm.height;
    vector<float> surface(cells);
    if (contour_surface == "dsm") {
        o3dr_raster_params rp;
        o3dr_raster_default_params(&rp);
        rp.cell_size = voxel_size, rp.select = O3DR_RASTER_TOP;
        rp.cx0 = prm.cx0, rp.cy0 = prm.cy0, rp.width = prm.width, rp.height = prm.height;
        vector<uint8_t> color(cells * 3);
        o3dr_raster_outputs out = {surface.data(), color.data(), nullptr, nullptr, nullptr};
        o3dr_raster_result res;
        chk(o3dr_rasterize_map(c, cloud->points.data(), n, &rp, &out, &res, O3DR_MEM_HOST), "o3dr_rasterize_map");
    } else {
        o3dr_ground_params gp;
        o3dr_ground_default_params(&gp);
        gp.cell_size = voxel_size;
        gp.cx0 = prm.cx0, gp.cy0 = prm.cy0, gp.width = prm.width, gp.height = prm.height;
        vector<uint8_t> ground((size_t)n);
        vector<float> dtm(cells);
        o3dr_ground_outputs out = {ground.data(), nullptr, dtm.data(), nullptr};
        o3dr_ground_result res;
        chk(o3dr_ground_filter(c, cloud->points.data(), n, &gp, &out, &res, O3DR_MEM_HOST), "o3dr_ground_filter");
        o3dr_interpolate_params ip;
        o3dr_interpolate_default_params(&ip);
        ip.width = prm.width, ip.height = prm.height;
        o3dr_interpolate_outputs io = {surface.data(), nullptr};
        o3dr_interpolate_result dem;
        chk(o3dr_raster_interpolate(c, dtm.data(), &ip, &io, &dem, O3DR_MEM_HOST), "o3dr_raster_interpolate");
    }
    const auto t0 = chrono::steady_clock::now();
    int64_t S = 0;
    chk(o3dr_raster_contours_count(c, surface.data(), &prm, &S, O3DR_MEM_HOST), "o3dr_raster_contours_count");
    if (S > (int64_t)O3DR_CONTOUR_MAX_SEGMENTS) throw runtime_error("more than 2^28 contour segments: --contour_interval is too small for this surface");
    vector<o3dr_contour_line> lines((size_t)S);  // n_lines <= n_segments, n_vertices <= 2 n_segments
    vector<double> vertices((size_t)S * 4);
    o3dr_contour_outputs out = {nullptr, 0, S ? lines.data() : nullptr, S, S ? vertices.data() : nullptr, 2 * S};
    o3dr_contour_result res;
    chk(o3dr_raster_contours(c, surface.data(), &prm, &out, &res, O3DR_MEM_HOST), "o3dr_raster_contours");
    const double ms = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
    const string path = next_to(read_PLY_filename0, "contours_", ".geojson");
    ofstream js(path);
    char num[96];
    int64_t written = 0;
    js << "{\"type\": \"FeatureCollection\", \"features\": [";
    for (int64_t l = 0; l < res.n_lines; ++l) {
        const o3dr_contour_line& ln = lines[(size_t)l];
        if (ln.n_segments < contour_min_segments) continue;
        snprintf(num, sizeof num, "%.17g", ln.level);
        js << (written++ ? ",\n" : "\n") << "{\"type\": \"Feature\", \"properties\": {\"line\": " << l << ", \"level\": " << ln.k << ", \"elevation\": " << num
           << ", \"closed\": " << ln.closed << ", \"segments\": " << ln.n_segments << "}, \"geometry\": {\"type\": \"LineString\", \"coordinates\": [";
        for (int64_t v = ln.begin; v <= ln.begin + ln.n_segments; ++v) {
            snprintf(num, sizeof num, "[%.17g, %.17g]", vertices[(size_t)v * 2], vertices[(size_t)v * 2 + 1]);
            js << (v > ln.begin ? ", " : "") << num;
        }
        js << "]}}";
    }
    js << "\n]}\n";
    js.close();
    if (!js) throw runtime_error("could not write " + path);
    char line[128];
    cout << "points in " << n << ", surface " << contour_surface << endl;
    cout << "box cx0 " << prm.cx0 << " cy0 " << prm.cy0 << " width " << prm.width << " height " << prm.height << endl;
    snprintf(line, sizeof line, "levels k %d .. %d (interval %.17g base %.17g)", res.k_lo, res.k_hi, contour_interval, contour_base);
    cout << line << endl;
    cout << "quads " << res.n_quads << " (crossed " << res.n_quads_crossed << "), segments " << res.n_segments << ", lines " << res.n_lines
         << " (closed " << res.n_closed << ", longest " << res.n_longest << " segments), vertices " << res.n_vertices << endl;
    snprintf(line, sizeof line, "contour time %.3f ms", ms);
    cout << line << endl;
    cerr << "Saved " << written << " contour lines to " << path << endl;
}

o3dr_orb_params Pose::orb_params() const
{
    o3dr_orb_params p;
    o3dr_orb_default_params(&p);
    p.n_features = orb_n_features;
    p.n_levels = orb_levels;
    p.scale_factor = orb_scale;
    p.fast_threshold = orb_fast_threshold;
    return p;
}

// findFeatures' first half for one image (pose.cpp:127,210: OpenCV's OrbFeaturesFinder), here o3dr_orb_detect (contract:
// include/o3dr.h "ORB features").  Prints the keypoints per pyramid level and writes KeyPoint::pt, one "x y" per line with
// %.9g (a float's exact round trip), as <image>.keypoints.txt: what --keypoints_dir reads as <img_num>.txt.
void Pose::run_find_features()
{
    const Image8 im = read_png(find_features_png, false);
    if (im.empty()) throw runtime_error("could not read " + find_features_png);
    const o3dr_orb_params prm = orb_params();
    const int64_t cap = prm.n_features > 0 ? prm.n_features : 1;
    vector<o3dr_orb_keypoint> kp((size_t)cap);
    vector<float> xy((size_t)cap * 2);
    int64_t off[2] = {0, 0}, n = 0;
    o3dr_ctx* c = ctx_for_this_thread();
    chk(o3dr_orb_detect(c, im.data.data(), 0, im.pitch(), im.rows, im.cols, 1, &prm, kp.data(), xy.data(), nullptr, off, nullptr, cap, &n,
                        O3DR_MEM_HOST),
        "o3dr_orb_detect");
    vector<int64_t> per_level((size_t)(prm.n_levels > 0 ? prm.n_levels : 1), 0);
    for (int64_t i = 0; i < n; ++i) per_level[kp[(size_t)i].level]++;
    cout << "image " << im.rows << " x " << im.cols << ", keypoints " << n << endl;
    for (size_t l = 0; l < per_level.size(); ++l) cout << "level " << l << ": " << per_level[l] << endl;
    const string outp = find_features_png + ".keypoints.txt";
    FILE* f = fopen(outp.c_str(), "w");
    if (!f) throw runtime_error("could not write " + outp);
    for (int64_t i = 0; i < n; ++i) fprintf(f, "%.9g %.9g\n", xy[(size_t)(2 * i)], xy[(size_t)(2 * i + 1)]);
    fclose(f);
    cerr << "Saved " << n << " keypoints to " << outp << endl;
}

o3dr_stereo_params Pose::stereo_params(int channels) const
{
    o3dr_stereo_params prm;
    o3dr_stereo_default_params(&prm);
    prm.n_disparities = stereo_n_disparities;
    prm.min_disparity = stereo_min_disparity;
    prm.p1 = stereo_p1;
    prm.p2 = stereo_p2;
    prm.n_paths = stereo_paths;
    prm.uniqueness = stereo_uniqueness;
    prm.lr_max_diff = stereo_lr_max_diff;
    prm.channels = channels;
    return prm;
}

// The disparity image of one rectified pair from o3dr_stereo_disparity (contract: include/o3dr.h "stereo disparity"),
// written as <left>.disparity.png: what --disparity_dir reads as <img_num>.png.
void Pose::run_stereo_disparity()
{
    Image8 left = read_png(stereo_left_png, false), right = read_png(stereo_right_png, false);
    if (left.empty()) throw runtime_error("could not read " + stereo_left_png);
    if (right.empty()) throw runtime_error("could not read " + stereo_right_png);
    if (left.rows != right.rows || left.cols != right.cols) throw runtime_error("--stereo_disparity: the two images differ in size");
    const o3dr_stereo_params prm = stereo_params(3);
    vector<uint8_t> disp((size_t)left.rows * left.cols);
    o3dr_ctx* c = ctx_for_this_thread();
    const auto t0 = chrono::steady_clock::now();
    if (!rectify_calib.empty()) {  // the matcher takes the rectified pair
        rectify_images(c, 0, {&left}, nullptr);
        rectify_images(c, 1, {&right}, nullptr);
    }
    chk(o3dr_stereo_disparity(c, left.data.data(), right.data.data(), 0, left.pitch(), left.rows, left.cols, 1, &prm, disp.data(), nullptr,
                              nullptr, nullptr, O3DR_MEM_HOST),
        "o3dr_stereo_disparity");
    o3dr_disparity_filter_info info = {};
    if (disparity_filter_on()) filter_disparities(c, disp, left.rows, left.cols, 1, &info);
    const double ms = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
    size_t accepted = 0;
    for (uint8_t d : disp) accepted += d != 0;
    cout << "pair " << left.rows << " x " << left.cols << ", disparities " << prm.min_disparity << ".." << prm.min_disparity + prm.n_disparities - 1
         << ", accepted " << accepted << " of " << disp.size() << " pixels";
    if (stereo_speckle_size > 0) cout << ", removed " << info.n_removed << " pixels in " << info.n_speckles << " speckles";
    cout << ", " << ms << " ms" << endl;
    const string outp = stereo_left_png + ".disparity.png";
    if (!write_png_grey8(outp, disp.data(), left.rows, left.cols)) throw runtime_error("could not write " + outp);
    cerr << "Saved the disparity image to " << outp << endl;
}

void Pose::filter_disparities(o3dr_ctx* c, vector<uint8_t>& disp, int rows, int cols, int n_frames, o3dr_disparity_filter_info* info)
{
    o3dr_disparity_filter_params prm;
    o3dr_disparity_filter_default_params(&prm);
    prm.median_size = stereo_median;
    prm.max_speckle_size = stereo_speckle_size;
    prm.max_diff = stereo_speckle_diff;
    const size_t n = (size_t)rows * cols;
    vector<uint8_t> out(n * (size_t)n_frames);
    chk(o3dr_disparity_filter(c, disp.data(), (int64_t)n, cols, rows, cols, n_frames, &prm, out.data(), nullptr, nullptr, info, O3DR_MEM_HOST),
        "o3dr_disparity_filter");
    copy(out.begin(), out.end(), disp.begin());
}

// The filter alone on an 8-bit grey PNG (contract: include/o3dr.h "disparity filter"), written as <in>.filtered.png.
void Pose::run_filter_disparity()
{
    const Image8 in = read_png(filter_disparity_png, true);
    if (in.empty() || in.channels != 1) throw runtime_error("could not read " + filter_disparity_png + " as an 8-bit grey PNG");
    vector<uint8_t> disp(in.data.begin(), in.data.begin() + (long)((size_t)in.rows * in.cols));
    o3dr_ctx* c = ctx_for_this_thread();
    o3dr_disparity_filter_info info = {};
    const auto t0 = chrono::steady_clock::now();
    filter_disparities(c, disp, in.rows, in.cols, 1, &info);
    const double ms = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
    cout << "image " << in.rows << " x " << in.cols << ", " << info.n_valid << " valid pixels in " << info.n_components
         << " components (largest " << info.largest << "), removed " << info.n_removed << " pixels in " << info.n_speckles << " speckles, "
         << ms << " ms" << endl;
    const string outp = filter_disparity_png + ".filtered.png";
    if (!write_png_grey8(outp, disp.data(), in.rows, in.cols)) throw runtime_error("could not write " + outp);
    cerr << "Saved the filtered image to " << outp << endl;
}

o3dr_segment_params Pose::segment_params(int channels) const
{
    o3dr_segment_params prm;
    o3dr_segment_default_params(&prm);
    prm.channels = channels;
    prm.step = segment_step, prm.compactness = segment_compactness, prm.iterations = segment_iterations, prm.min_size = segment_min_size;
    return prm;
}

// Superpixel labels of one image (contract: include/o3dr.h "image segmentation"), written as <image>.labels.png, 16-bit grey.
void Pose::run_segment_image()
{
    const Image8 in = read_png(segment_image_png, false);
    if (in.empty() || (in.channels != 1 && in.channels != 3)) throw runtime_error("could not read " + segment_image_png + " as an 8-bit PNG");
    const size_t n = (size_t)in.rows * in.cols;
    const o3dr_segment_params prm = segment_params(in.channels);
    vector<int32_t> labels(n);
    o3dr_segment_info info = {};
    o3dr_ctx* c = ctx_for_this_thread();
    const auto t0 = chrono::steady_clock::now();
    chk(o3dr_segment_image(c, in.data.data(), 0, in.pitch(), in.rows, in.cols, 1, &prm, labels.data(), nullptr, nullptr, &info, O3DR_MEM_HOST),
        "o3dr_segment_image");
    const double ms = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
    cout << "image " << in.rows << " x " << in.cols << ", " << info.n_centres << " centres, " << info.n_components << " components, "
         << info.n_merged << " merged, " << info.n_labels << " labels (largest " << info.largest << ", smallest " << info.smallest << "), "
         << ms << " ms" << endl;
    if (info.n_labels > 65536) throw runtime_error("more than 65536 labels: a 16-bit label image cannot hold them");
    vector<uint16_t> lab16(n);
    for (size_t i = 0; i < n; ++i) lab16[i] = (uint16_t)labels[i];
    const string outp = segment_image_png + ".labels.png";
    if (!write_png_grey16(outp, lab16.data(), in.rows, in.cols)) throw runtime_error("could not write " + outp);
    cerr << "Saved the label image to " << outp << endl;
}

// --gpu_segment_labels: every frame's label image from o3dr_segment_image on its rgb image (as it is after --rectify_calib),
// the frames of one size in calls of up to 16.  A frame with more than 65536 labels, or whose rgb image is not of its
// disparity image's size, is left without a label image and is rejected like one whose label PNG could not be read.
void Pose::compute_gpu_segment_labels()
{
    vector<RawImageData*> todo;
    int prows = 0, pcols = 0;
    for (RawImageData& r : rawImageDataVec) {
        r.label_image = Image16();
        if (r.rgb_image.empty() || r.rgb_image.channels != 3) continue;
        if (!prows) prows = r.rgb_image.rows, pcols = r.rgb_image.cols;
        if (r.rgb_image.rows == prows && r.rgb_image.cols == pcols) todo.push_back(&r);
    }
    if (todo.empty()) return;
    const o3dr_segment_params prm = segment_params(3);
    const size_t per_call = (size_t)min(seq_len > 0 ? seq_len : 16, 16), n = (size_t)prows * pcols;
    vector<uint8_t> img(per_call * n * 3);
    vector<int32_t> labels(per_call * n);
    vector<o3dr_segment_info> info(per_call);
    o3dr_ctx* c = ctx_for_this_thread();
    size_t n_made = 0;
    for (size_t k0 = 0; k0 < todo.size(); k0 += per_call) {
        const size_t k1 = min(todo.size(), k0 + per_call);
        for (size_t k = k0; k < k1; ++k) memcpy(&img[(k - k0) * n * 3], todo[k]->rgb_image.data.data(), n * 3);
        chk(o3dr_segment_image(c, img.data(), (int64_t)(n * 3), 3 * (int64_t)pcols, prows, pcols, (int32_t)(k1 - k0), &prm, labels.data(),
                               nullptr, nullptr, info.data(), O3DR_MEM_HOST),
            "o3dr_segment_image");
        for (size_t k = k0; k < k1; ++k) {
            RawImageData& r = *todo[k];
            if (info[k - k0].n_labels > 65536) continue;
            if (!r.disparity_image.empty() && (r.disparity_image.rows != prows || r.disparity_image.cols != pcols)) continue;
            Image16& li = r.label_image;
            li.rows = prows, li.cols = pcols;
            li.data.resize(n);
            for (size_t i = 0; i < n; ++i) li.data[i] = (uint16_t)labels[(k - k0) * n + i];
            ++n_made;
        }
    }
    cout << "--gpu_segment_labels: " << n_made << " label images from o3dr_segment_image" << endl;
}

// Images of one size through camera `cam`'s map of that size (o3dr_rectify_maps, kept until another size is asked for) in
// one o3dr_rectify_remap call; the output size equals the input size.
void Pose::rectify_images(o3dr_ctx* c, int cam, const vector<Image8*>& imgs, int64_t* n_valid)
{
    if (imgs.empty()) return;
    const int rows = imgs[0]->rows, cols = imgs[0]->cols, ch = imgs[0]->channels;
    const size_t n = (size_t)rows * cols, F = imgs.size();
    RectifyMap& m = rectify_map[cam];
    if (m.rows != rows || m.cols != cols) {
        m.map.assign(n * 2, 0);
        m.rows = m.cols = 0;
        chk(o3dr_rectify_maps(c, &rectify_cam[cam], rows, cols, m.map.data(), O3DR_MEM_HOST), "o3dr_rectify_maps");
        m.rows = rows, m.cols = cols;
    }
    vector<uint8_t> src(F * n * ch), out(F * n * ch), valid(n_valid ? n : 0);
    for (size_t k = 0; k < F; ++k) memcpy(&src[k * n * ch], imgs[k]->data.data(), n * ch);
    chk(o3dr_rectify_remap(c, src.data(), (int64_t)(n * ch), (int64_t)cols * ch, rows, cols, ch, (int32_t)F, m.map.data(), rows, cols,
                           rectify_border, 0, out.data(), n_valid ? valid.data() : nullptr, O3DR_MEM_HOST),
        "o3dr_rectify_remap");
    for (size_t k = 0; k < F; ++k) memcpy(imgs[k]->data.data(), &out[k * n * ch], n * ch);
    if (n_valid) {
        *n_valid = 0;
        for (uint8_t v : valid) *n_valid += v;
    }
}

// One raw pair through o3dr_rectify_maps and o3dr_rectify_remap (contract: include/o3dr.h "stereo rectification"), written
// as <left>.rectified.png and <right>.rectified.png: what --stereo_disparity, image_dir and right_image_dir take.
void Pose::run_rectify_pair()
{
    Image8 im[2] = {read_png(rectify_left_png, false), read_png(rectify_right_png, false)};
    const string* path[2] = {&rectify_left_png, &rectify_right_png};
    for (int k = 0; k < 2; ++k)
        if (im[k].empty()) throw runtime_error("could not read " + *path[k]);
    if (im[0].rows != im[1].rows || im[0].cols != im[1].cols) throw runtime_error("--rectify_pair: the two images differ in size");
    o3dr_ctx* c = ctx_for_this_thread();
    int64_t n_valid[2] = {0, 0};
    const auto t0 = chrono::steady_clock::now();
    for (int k = 0; k < 2; ++k) rectify_images(c, k, {&im[k]}, &n_valid[k]);
    const double ms = chrono::duration<double, milli>(chrono::steady_clock::now() - t0).count();
    cout << "pair " << im[0].rows << " x " << im[0].cols << ", valid " << n_valid[0] << " (left) and " << n_valid[1] << " (right) of "
         << (size_t)im[0].rows * im[0].cols << " pixels, " << ms << " ms" << endl;
    for (int k = 0; k < 2; ++k) {
        const string outp = *path[k] + ".rectified.png";
        const bool ok = im[k].channels == 3 ? write_png_bgr8(outp, im[k].data.data(), im[k].rows, im[k].cols)
                                            : write_png_grey8(outp, im[k].data.data(), im[k].rows, im[k].cols);
        if (!ok) throw runtime_error("could not write " + outp);
        cerr << "Saved the rectified image to " << outp << endl;
    }
}

// --rectify_calib in a reconstruction run: every readable rgb_image - under --gpu_disparity every right_image too - is
// replaced by its rectified version, a cycle's frames (at most 16) of one size per call and camera.  Colours, keypoints,
// feature poses and the GPU matcher all see the rectified images; a disparity image read from --disparity_dir is taken to
// be in rectified coordinates already.
void Pose::rectify_raw_images()
{
    const size_t per_call = (size_t)min(seq_len > 0 ? seq_len : 16, 16);
    o3dr_ctx* c = ctx_for_this_thread();
    size_t done[2] = {0, 0};
    for (int cam = 0; cam < (gpu_disparity ? 2 : 1); ++cam) {
        vector<Image8*> batch;
        auto flush = [&]() {
            rectify_images(c, cam, batch, nullptr);
            done[cam] += batch.size();
            batch.clear();
        };
        for (RawImageData& r : rawImageDataVec) {
            Image8& im = cam == 0 ? r.rgb_image : r.right_image;
            if (im.empty()) continue;
            if (!batch.empty() && (batch.size() == per_call || batch[0]->rows != im.rows || batch[0]->cols != im.cols)) flush();
            batch.push_back(&im);
        }
        flush();
    }
    cout << "--rectify_calib: " << done[0] << " left" << (gpu_disparity ? " and " + to_string(done[1]) + " right" : string())
         << " images rectified by o3dr_rectify_remap" << endl;
}

// --gpu_disparity: where the disparity PNGs would have been read, every raw frame with a readable pair gets its disparity
// image from o3dr_stereo_disparity, a cycle's frames (at most 16) per call; the variance gate, the blur and everything
// after them see that image.  A frame whose pair is unreadable or of another size than the first pair keeps no
// disparity image and is rejected like one whose PNG is missing.
void Pose::compute_gpu_disparities()
{
    vector<RawImageData*> todo;
    int prows = 0, pcols = 0;
    for (RawImageData& r : rawImageDataVec) {
        if (r.rgb_image.empty() || r.right_image.empty()) continue;
        if (!prows) prows = r.rgb_image.rows, pcols = r.rgb_image.cols;
        if (r.rgb_image.rows == prows && r.rgb_image.cols == pcols && r.right_image.rows == prows && r.right_image.cols == pcols)
            todo.push_back(&r);
    }
    if (todo.empty()) return;
    const o3dr_stereo_params prm = stereo_params(3);
    const size_t per_call = (size_t)min(seq_len > 0 ? seq_len : 16, 16), n = (size_t)prows * pcols;
    vector<uint8_t> left(per_call * n * 3), right(per_call * n * 3), disp(per_call * n);
    o3dr_ctx* c = ctx_for_this_thread();
    for (size_t k0 = 0; k0 < todo.size(); k0 += per_call) {
        const size_t k1 = min(todo.size(), k0 + per_call);
        for (size_t k = k0; k < k1; ++k) {
            memcpy(&left[(k - k0) * n * 3], todo[k]->rgb_image.data.data(), n * 3);
            memcpy(&right[(k - k0) * n * 3], todo[k]->right_image.data.data(), n * 3);
        }
        chk(o3dr_stereo_disparity(c, left.data(), right.data(), (int64_t)(n * 3), 3 * (int64_t)pcols, prows, pcols, (int32_t)(k1 - k0), &prm,
                                  disp.data(), nullptr, nullptr, nullptr, O3DR_MEM_HOST),
            "o3dr_stereo_disparity");
        if (disparity_filter_on()) filter_disparities(c, disp, prows, pcols, (int)(k1 - k0), nullptr);  // (disp's first k1 - k0 frames)
        for (size_t k = k0; k < k1; ++k) {
            Image8& d = todo[k]->disparity_image;
            d.rows = prows, d.cols = pcols, d.channels = 1;
            d.data.assign(disp.begin() + (long)((k - k0) * n), disp.begin() + (long)((k - k0 + 1) * n));
            todo[k]->right_image = Image8();
        }
    }
    cout << "--gpu_disparity: " << todo.size() << " disparity images from o3dr_stereo_disparity"
         << (disparity_filter_on() ? ", filtered by o3dr_disparity_filter" : "") << endl;
}

// pose.cpp:23-565 restricted to the hot path
Pose::Pose(int argc, char* argv[])
{
    if (parseCmdArgs(argc, argv) != 0) return;
    if (!run3d_reconstruction) Q = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};  // a tool needs no camera
    if (downsample) {  // pose.cpp:71-87
        PointCloud::Ptr cloud = read_PLY_File(read_PLY_filename0);
        PointCloud::Ptr small = downsamplePtCloud(cloud, true);
        string out = next_to(read_PLY_filename0, "downsampled_");
        save_pt_cloud_to_PLY_File(small, out);
        return;
    }
    if (align_point_cloud) {
        run_align_point_cloud();
        return;
    }
    if (smooth_surface) {
        run_smooth_surface();
        return;
    }
    if (segment_cloud_only) {
        run_segment_cloud();
        return;
    }
    if (mesh_surface) {
        run_mesh_surface();
        return;
    }
    if (orthophoto) {
        run_orthophoto();
        return;
    }
    if (ground_filter) {
        run_ground_filter();
        return;
    }
    if (cluster_cloud) {
        run_cluster_cloud();
        return;
    }
    if (contours) {
        run_contours();
        return;
    }
    if (!find_features_png.empty()) {
        run_find_features();
        return;
    }
    if (!stereo_left_png.empty()) {
        run_stereo_disparity();
        return;
    }
    if (!rectify_left_png.empty()) {
        run_rectify_pair();
        return;
    }
    if (!filter_disparity_png.empty()) {
        run_filter_disparity();
        return;
    }
    if (!segment_image_png.empty()) {
        run_segment_image();
        return;
    }
    if (!print_label_png.empty()) {  // what read_png_labels makes of one file: "rows cols", then one row of labels per line
        const Image16 im = read_png_labels(print_label_png);
        if (im.empty()) throw runtime_error("could not read " + print_label_png + " as an 8- or 16-bit greyscale PNG");
        cout << im.rows << " " << im.cols << "\n";
        for (int y = 0; y < im.rows; ++y) {
            for (int x = 0; x < im.cols; ++x) cout << (x ? " " : "") << im.data[(size_t)y * im.cols + x];
            cout << "\n";
        }
        return;
    }
    if (!run3d_reconstruction) return;
    populateData();
    if (rows == 0 || cols == 0 || cols_start_aft_cutout == 0)
        throw "Exception: some important values not set! rows/cols/cols_start_aft_cutout";
    run_reconstruction();
}

// ------------------------------------------------------------------------------------------------
// the reconstruction run: every cycle accepts frames, stacks the accepted ones in one batch and takes
// the batch through the stages below into cloud_big (pose.cpp:162-434)
// ------------------------------------------------------------------------------------------------
typedef chrono::steady_clock clk;

// The frames [first, last) of the accepted list, stacked as the batched calls take them.  While the batch lives its two
// image stacks are page-locked, so that they cross PCIe by DMA (best effort: pageable memory works too, through the
// runtime's bounce buffers; only what was registered is released).  The stacks never change size.
struct Pose::FrameBatch {
    size_t first, n;          // the batch's first frame in the accepted list, the frames stacked
    size_t n_cloud;           // the frames that go into the cloud, the first n_cloud of the stacks: n until the pose chain drops some
    size_t dsz = 0, csz = 0;  // bytes of one 8-bit disparity image and of one colour image
    vector<uint8_t> disp, bgr;
    vector<float> poses, kp_xy;
    vector<int64_t> kp_off;
    bool reg_disp = false, reg_bgr = false;

    FrameBatch(const vector<ImageData>& accepted, size_t first_, size_t last) : first(first_), n(last - first_), n_cloud(n), poses(16 * n), kp_off(n + 1, 0)
    {
        const RawImageData& r0 = *accepted[first].raw_img_data_ptr;
        dsz = r0.disparity_image.data.size(), csz = r0.rgb_image.data.size();
        disp.resize(dsz * n), bgr.resize(csz * n);
        for (size_t k = 0; k < n; ++k) {
            const ImageData& im = accepted[first + k];
            memcpy(&disp[k * dsz], im.raw_img_data_ptr->disparity_image.data.data(), dsz);
            memcpy(&bgr[k * csz], im.raw_img_data_ptr->rgb_image.data.data(), csz);
            memcpy(&poses[16 * k], im.t_mat_FeatureMatched.data(), 64);
            kp_xy.insert(kp_xy.end(), im.keypoints_xy.begin(), im.keypoints_xy.end());
            kp_off[k + 1] = (int64_t)(kp_xy.size() / 2);
        }
        reg_disp = o3dr_host_register(disp.data(), (int64_t)disp.size()) == O3DR_OK;
        reg_bgr = o3dr_host_register(bgr.data(), (int64_t)bgr.size()) == O3DR_OK;
    }
    FrameBatch(const FrameBatch&) = delete;
    ~FrameBatch()
    {
        if (reg_disp) (void)o3dr_host_unregister(disp.data());
        if (reg_bgr) (void)o3dr_host_unregister(bgr.data());
    }
};

// disparity_f64 on, and pushed, while this lives: the accumulate call then takes float64 images (the plane fits, the fused
// levels).  Off and pushed again at the end of the scope, on the error path too.
struct Pose::F64Images {
    Pose& p;
    o3dr_ctx* c;
    F64Images(Pose& p_, o3dr_ctx* c_) : p(p_), c(c_)
    {
        p.disparity_f64 = true;
        p.push_params(c);
    }
    ~F64Images()
    {
        p.disparity_f64 = false;
        try {
            p.push_params(c);  // (the values that went through at the start of the run)
        } catch (...) {
        }
    }
};

// What a cycle's stages hand on to the later ones
struct Pose::CycleState {
    vector<float> orb_xy;           // stage 1: the batch's ORB keypoints, their descriptors (--feature_poses) and row offsets per frame
    vector<uint8_t> orb_desc;
    vector<int64_t> orb_off;
    vector<double> fitted, fused;   // the plane-fitted images (stage 2), the fused levels (stage 5)
    uint8_t* disp_in = nullptr;     // the disparity stack the pose chain reads and the compaction moves, esz bytes per pixel
    const uint8_t* acc_in = nullptr;  // the one the accumulate call takes, acc_esz bytes per pixel
    int64_t esz = 1, acc_esz = 1;
    vector<o3dr_chain_frame> recs;  // stage 3 for stage 4: the chain's records, poses and dropped counts, history + batch
    vector<float> chain_poses;
    vector<int64_t> dropped;
    optional<F64Images> f64;        // (last: restored before anything above goes)
};

// A stage's failed library call ends the cycle: "accumulate_frames: <stage><library message>".  Called before any guard makes
// a library call of its own (o3dr_host_unregister, o3dr_set_params), which may overwrite o3dr_last_error().
static void stage_chk(int rc, const char* stage)
{
    if (rc != O3DR_OK) throw runtime_error(string("accumulate_frames: ") + stage + o3dr_last_error());
}

// Stage 1, --gpu_keypoints and / or --feature_poses: the batch's ORB features from one extractor call.  With --gpu_keypoints,
// jump_pixels != 1 and no --keypoints_dir they are the batch's keypoint lists, instead of files (the list the reference's
// ORB stage leaves in features.keypoints, pose_functions.cpp:1057-1061).
void Pose::orb_stage(o3dr_ctx* c, FrameBatch& b, CycleState& s)
{
    const bool orb_for_cloud = gpu_keypoints && jump_pixels != 1 && keypointsPrefix.empty();
    if (!orb_for_cloud && !feature_poses) return;
    const o3dr_orb_params prm = orb_params();
    const int64_t cap = (int64_t)b.n * (prm.n_features > 0 ? prm.n_features : 1);
    s.orb_xy.assign((size_t)cap * 2, 0.f);
    if (feature_poses) s.orb_desc.assign((size_t)cap * 32, 0);
    s.orb_off.assign(b.n + 1, 0);
    int64_t n_kp = 0;
    const auto tk = clk::now();
    const int rc = o3dr_orb_detect(c, b.bgr.data(), (int64_t)b.csz, 3 * (int64_t)cols, rows, cols, (int32_t)b.n, &prm, nullptr, s.orb_xy.data(),
                                   feature_poses ? s.orb_desc.data() : nullptr, s.orb_off.data(), nullptr, cap, &n_kp, O3DR_MEM_HOST);
    cout << "\nORB keypoints: " << n_kp << " in " << b.n << " frames, " << chrono::duration<double>(clk::now() - tk).count() << " sec"
         << flush;  // (of a failed call too; printing is no library call)
    stage_chk(rc, "orb_detect: ");
    s.orb_xy.resize((size_t)n_kp * 2);
    s.orb_desc.resize(feature_poses ? (size_t)n_kp * 32 : 0);
    if (orb_for_cloud) {
        b.kp_xy = s.orb_xy;
        b.kp_off = s.orb_off;
    }
}

// Stage 2, --use_segment_labels: the batch's 8-bit disparities become plane-fitted CV_64F images, which every later stage
// takes in their place
void Pose::plane_fit_stage(o3dr_ctx* c, FrameBatch& b, CycleState& s)
{
    if (!use_segment_labels) return;
    vector<uint16_t> lab(b.dsz * b.n);
    uint32_t max_label = 0;
    for (size_t k = 0; k < b.n; ++k) {
        const Image16& li = acceptedImageDataVec[b.first + k].raw_img_data_ptr->label_image;
        memcpy(&lab[k * b.dsz], li.data.data(), b.dsz * sizeof(uint16_t));
        for (uint16_t v : li.data) max_label = max<uint32_t>(max_label, v);
    }
    s.fitted.resize(b.dsz * b.n);
    o3dr_plane_disp_params pp;
    o3dr_plane_disp_default_params(&pp);
    pp.min_pixels = plane_min_pixels;
    pp.max_mse = plane_max_mse;
    const auto tf = clk::now();
    const int rc = o3dr_plane_fit_disparity(c, b.disp.data(), cols, (int64_t)b.dsz, lab.data(), 2, 2 * (int64_t)cols, 2 * (int64_t)b.dsz,
                                            (int32_t)max_label + 1, rows, cols, (int32_t)b.n, &pp, s.fitted.data(), nullptr, nullptr,
                                            O3DR_MEM_HOST);
    cout << "\nplane-fitted disparity: " << b.n << " frames, " << max_label + 1 << " labels, "
         << chrono::duration<double>(clk::now() - tf).count() << " sec" << flush;  // (of a failed call too)
    stage_chk(rc, "plane_fit_disparity: ");
    s.f64.emplace(*this, c);
    s.acc_in = s.disp_in = (uint8_t*)s.fitted.data();
    s.acc_esz = s.esz = 8;
}

// Stage 3, --feature_poses: the batch's frames through the chain, the frames of the cycles before as its history; with
// --refine_poses then one joint refinement of the batch's matched frames over the batch's pairs, the history held
void Pose::pose_chain_stage(o3dr_ctx* c, FrameBatch& b, CycleState& s)
{
    if (!feature_poses) return;
    const auto tc = clk::now();
    const size_t n_hist = chain.status.size(), n_all = n_hist + b.n, n_kp = s.orb_xy.size() / 2;
    vector<o3dr_point> kp3(n_kp ? n_kp : 1);
    int64_t n3 = 0;
    stage_chk(o3dr_keypoints_3d(c, s.disp_in, s.esz * (int64_t)b.dsz, s.esz * cols, nullptr, 0, 0, rows, cols, nullptr, (int32_t)b.n,
                                s.orb_xy.data(), s.orb_off.data(), kp3.data(), (int64_t)kp3.size(), &n3, O3DR_MEM_HOST),
              "keypoints_3d: ");
    const int64_t base = chain.off.back();
    chain.desc.insert(chain.desc.end(), s.orb_desc.begin(), s.orb_desc.end());
    chain.kp3.insert(chain.kp3.end(), kp3.begin(), kp3.begin() + (ptrdiff_t)n_kp);
    for (size_t k = 0; k < b.n; ++k) {
        chain.off.push_back(base + s.orb_off[k + 1]);
        const Matrix4& m = acceptedImageDataVec[b.first + k].t_mat_MAVLink;
        chain.prior.insert(chain.prior.end(), m.begin(), m.end());
    }
    s.chain_poses.resize(16 * n_all);
    s.recs.resize(n_all);
    o3dr_chain_params cp;
    o3dr_chain_default_params(&cp);
    cp.dist_nearby = dist_nearby;
    cp.range_width = range_width;
    cp.min_matches = chain_min_matches;
    cp.max_rms = chain_max_rms;
    // --chain_ransac_threshold: the pair list and one RANSAC record per pair come back too, for the dropped counts
    o3dr_ransac_params rp;
    o3dr_ransac_default_params(&rp);
    rp.threshold = chain_ransac_threshold;
    rp.iterations = chain_ransac_iterations;
    rp.seed = chain_ransac_seed;
    const bool want_pairs = chain_ransac || refine_poses;
    const size_t pair_cap = want_pairs ? b.n * (size_t)O3DR_CHAIN_MAX_RANGE : 0;
    vector<int32_t> pair_list(2 * pair_cap + 2);
    vector<o3dr_ransac_result> rres(pair_cap + 1);
    int64_t n_list = 0;
    stage_chk(o3dr_pose_chain_robust(c, chain.desc.data(), chain.off.data(), chain.kp3.data(), chain.prior.data(), (int32_t)n_all,
                                     (int32_t)n_hist, chain.poses.data(), chain.status.data(), &cp, s.chain_poses.data(), s.recs.data(),
                                     want_pairs ? pair_list.data() : nullptr, (int64_t)pair_cap, &n_list, O3DR_MEM_HOST,
                                     chain_ransac ? &rp : nullptr, chain_ransac ? rres.data() : nullptr),
              "pose_chain: ");
    // a frame's dropped slots: over its pairs with an accepted train frame, the candidates that are no inliers
    s.dropped.assign(n_all, 0);
    for (int64_t k = 0; chain_ransac && k < n_list; ++k) {
        const int32_t st_j = s.recs[(size_t)pair_list[2 * (size_t)k + 1]].status;
        if (st_j == O3DR_CHAIN_ANCHOR || st_j == O3DR_CHAIN_MATCHED)
            s.dropped[(size_t)pair_list[2 * (size_t)k]] += rres[(size_t)k].n_candidates - rres[(size_t)k].n_inliers;
    }
    o3dr_refine_result rr = {};
    if (refine_poses) {
        vector<int32_t> st_all(n_all);
        vector<uint8_t> held(n_all, 0);
        for (size_t f = 0; f < n_all; ++f) st_all[f] = s.recs[f].status, held[f] = f < n_hist;
        vector<float> refined(16 * n_all);
        vector<o3dr_refine_frame> rfr(n_all);
        o3dr_refine_params fp;
        o3dr_refine_default_params(&fp);
        fp.gn_iterations = refine_gn_iterations;
        fp.cg_iterations = refine_cg_iterations;
        fp.prior_weight = refine_prior_weight;
        stage_chk(o3dr_pose_graph_refine(c, chain.desc.data(), chain.off.data(), chain.kp3.data(), (int32_t)n_all, s.chain_poses.data(),
                                         st_all.data(), held.data(), chain.prior.data(), pair_list.data(), n_list, &fp,
                                         chain_ransac ? &rp : nullptr, refined.data(), rfr.data(), nullptr, &rr, O3DR_MEM_HOST),
                  "pose_graph_refine: ");
        s.chain_poses = refined;  // (a frame that is not free keeps its bytes)
    }
    chain.poses = s.chain_poses;
    cout << "\npose chain: " << b.n << " frames after " << n_hist << ", " << chrono::duration<double>(clk::now() - tc).count() << " sec" << endl;
    if (refine_poses)
        cout << "pose graph: edges " << rr.n_edges << " free " << rr.n_free << " energy " << rr.energy_before << " -> " << rr.energy_after
             << " gradient " << rr.grad_after << endl;
}

// Stage 4, --feature_poses: one status line per frame; a matched frame takes the chain's pose, a rejected one leaves the
// stacks: the accepted frames move up in place (m <= k)
void Pose::keep_chained_frames(FrameBatch& b, CycleState& s)
{
    if (!feature_poses) return;
    const size_t n_hist = chain.status.size(), fsz = b.dsz * (size_t)s.esz;
    size_t kp_rows = 0;
    b.n_cloud = 0;
    b.kp_off[0] = 0;
    for (size_t k = 0; k < b.n; ++k) {
        const o3dr_chain_frame& r = s.recs[n_hist + k];
        ImageData& im = acceptedImageDataVec[b.first + k];
        chain.status.push_back(r.status);
        memcpy(im.t_mat_FeatureMatched.data(), &s.chain_poses[16 * (n_hist + k)], 64);
        const bool ok = r.status == O3DR_CHAIN_ANCHOR || r.status == O3DR_CHAIN_MATCHED;
        cout << im.raw_img_data_ptr->img_num << " pose chain: " << kChainStatusName[r.status] << " pairs " << r.n_pairs_accepted << "/"
             << r.n_pairs << " good " << r.n_good << " used " << r.n_used << " rms " << r.rms;
        if (chain_ransac) cout << " dropped " << s.dropped[n_hist + k];
        cout << (ok ? "\tAccepted!" : "\tRejected!") << endl;
        if (!ok) continue;
        const size_t m = b.n_cloud++;
        const size_t r0k = (size_t)(b.kp_xy.empty() ? 0 : b.kp_off[k]), r1k = (size_t)(b.kp_xy.empty() ? 0 : b.kp_off[k + 1]);
        if (m != k) {
            memmove(s.disp_in + m * fsz, s.disp_in + k * fsz, fsz);
            memmove(&b.bgr[m * b.csz], &b.bgr[k * b.csz], b.csz);
        }
        memcpy(&b.poses[16 * m], im.t_mat_FeatureMatched.data(), 64);
        if (!b.kp_xy.empty()) memmove(&b.kp_xy[2 * kp_rows], &b.kp_xy[2 * r0k], (r1k - r0k) * 2 * sizeof(float));
        kp_rows += r1k - r0k;
        b.kp_off[m + 1] = (int64_t)kp_rows;
    }
    if (!b.kp_xy.empty()) b.kp_xy.resize(kp_rows * 2);
    cout << "Adding Point Cloud number/points: " << b.n_cloud << " of " << b.n << " frames" << flush;
}

// Stage 5, --multiview_filter / --multiview_fuse: the frames that go into the cloud, with their final poses, vote on each
// other's pixels; the fusion's float64 levels then go into the accumulate call in place of the 8-bit images
void Pose::multiview_stage(o3dr_ctx* c, FrameBatch& b, CycleState& s)
{
    if (!(multiview_filter || multiview_fuse) || b.n_cloud == 0) return;
    const char* const stage = multiview_fuse ? "multiview_fuse: " : "multiview_filter: ";
    const auto tm = clk::now();
    const size_t n = b.n_cloud;
    o3dr_multiview_params mp;
    o3dr_multiview_default_params(&mp);
    mp.tolerance = mv_tolerance;
    mp.min_support = mv_min_support;
    mp.max_violations = mv_max_violations;
    const int32_t nk = (int32_t)mv_neighbors;
    vector<int32_t> nb(n * (size_t)(nk > 0 && nk <= O3DR_MULTIVIEW_MAX_NEIGHBORS ? nk : 0) + 1);
    vector<o3dr_multiview_info> mi(n);
    int64_t n_pairs = 0, n_valid = 0, n_kept = 0, n_nosup = 0, n_viol = 0, n_votes = 0, n_fused = 0;
    stage_chk(o3dr_nearby_frames(b.poses.data(), (int32_t)n, nk, mv_max_distance, nb.data()), stage);
    if (multiview_fuse) {
        vector<o3dr_multiview_fuse_info> fi(n);
        s.fused.resize(b.dsz * n);
        stage_chk(o3dr_multiview_fuse(c, b.disp.data(), (int64_t)b.dsz, cols, rows, cols, (int32_t)n, b.poses.data(), nb.data(), nk, &mp,
                                      s.fused.data(), nullptr, nullptr, nullptr, fi.data(), O3DR_MEM_HOST),
                  stage);
        for (size_t f = 0; f < n; ++f) mi[f] = fi[f].filter, n_votes += fi[f].n_votes, n_fused += fi[f].n_fused;
        s.acc_in = (const uint8_t*)s.fused.data();
        s.acc_esz = 8;
        s.f64.emplace(*this, c);
    } else {
        vector<uint8_t> kept(b.dsz * n);
        stage_chk(o3dr_multiview_filter(c, b.disp.data(), (int64_t)b.dsz, cols, rows, cols, (int32_t)n, b.poses.data(), nb.data(), nk, &mp,
                                        kept.data(), nullptr, nullptr, mi.data(), O3DR_MEM_HOST),
                  stage);
        memcpy(b.disp.data(), kept.data(), kept.size());
    }
    for (size_t e = 0; e < n * (size_t)nk; ++e) n_pairs += nb[e] >= 0;
    for (const o3dr_multiview_info& m : mi) n_valid += m.n_valid, n_kept += m.n_kept, n_nosup += m.n_no_support, n_viol += m.n_violated;
    cout << "\nmultiview " << (multiview_fuse ? "fuse: " : "filter: ") << n << " frames, " << n_pairs << " pairs, kept " << n_kept << " of "
         << n_valid << " pixels (" << n_nosup << " without support, " << n_viol << " violated), ";
    if (multiview_fuse) cout << n_votes << " votes into " << n_fused << " pixels, ";
    cout << chrono::duration<double>(clk::now() - tm).count() << " sec" << flush;
}

// One cycle's accepted frames [first, last) into cloud_big.  MI355X-native form of the reference's loop over the frames
// (pose.cpp:365-434): the whole cycle in one batched call, cloud_big in HBM.
void Pose::accumulate_cycle(o3dr_ctx* c, size_t first, size_t last)
{
    FrameBatch b(acceptedImageDataVec, first, last);
    for (size_t k = first; k < last && !feature_poses; ++k) cout << " " << acceptedImageDataVec[k].raw_img_data_ptr->img_num << flush;
    CycleState s;  // (goes before the batch: disparity_f64 is restored, then the stacks are unpinned)
    s.acc_in = s.disp_in = b.disp.data();
    orb_stage(c, b, s);
    plane_fit_stage(c, b, s);
    pose_chain_stage(c, b, s);
    keep_chained_frames(b, s);
    multiview_stage(c, b, s);
    if (b.n_cloud == 0) return;
    stage_chk(o3dr_accumulate_frames_kp(c, s.acc_in, s.acc_esz * (int64_t)b.dsz, s.acc_esz * cols, b.bgr.data(), (int64_t)b.csz,
                                        3 * (int64_t)cols, rows, cols, b.poses.data(), (int32_t)b.n_cloud,
                                        b.kp_xy.empty() ? nullptr : b.kp_xy.data(), b.kp_xy.empty() ? nullptr : b.kp_off.data(), O3DR_MEM_HOST),
              "");
}

// The accept loop of one cycle (pose.cpp:162-255): up to cycle_len raw frames from current_idx on that can be read and pass
// the variance gate join the accepted list, with their recorded pose and, under --keypoints_dir, their keypoint file
void Pose::accept_cycle(int& current_idx, int cycle_len)
{
    const int last_idx = (int)rawImageDataVec.size() - 1;
    for (int images_in_cycle = 0; images_in_cycle < cycle_len && current_idx <= last_idx; current_idx++) {
        RawImageData& r = rawImageDataVec[current_idx];
        if (r.rgb_image.empty()) { cout << r.img_num << " could not read rgb image. \tRejected!" << endl; continue; }
        if (r.disparity_image.empty()) { cout << r.img_num << " could not read disparity image. \tRejected!" << endl; continue; }
        if (use_segment_labels && r.label_image.empty()) { cout << r.img_num << " could not read segment label image. \tRejected!" << endl; continue; }
        const double var = getVariance(r.disparity_image);
        cout << r.img_num << " " << flush;
        if (var > 5) { cout << " disp_img_var = " << var << " > 5.\tRejected!" << endl; continue; }
        ImageData d;
        d.raw_img_data_ptr = &r;
        d.t_mat_MAVLink = generateTmat(current_idx);
        d.t_mat_FeatureMatched = d.t_mat_MAVLink;  // --only_MAVLink, pose.cpp:238
        if (!keypointsPrefix.empty()) {
            // the list the reference's ORB stage would leave in features.keypoints (pose_functions.cpp:1057-1061)
            ifstream kf(keypointsPrefix + to_string(r.img_num) + ".txt");
            float kx, ky;
            while (kf >> kx >> ky) {
                d.keypoints_xy.push_back(kx);
                d.keypoints_xy.push_back(ky);
            }
        }
        acceptedImageDataVec.push_back(d);
        cout << "\tAccepted!" << endl;
        images_in_cycle++;
    }
}

// --reference_fanout, the reference's own structure: batches of <= 7 threads, results appended in frame order
void Pose::fanout_cycle(size_t first, size_t last, PointCloud& cloud_big_host)
{
    for (size_t i0 = first; i0 < last; i0 += 7) {
        const size_t nb = min<size_t>(7, last - i0);
        vector<PointCloud::Ptr> clouds(nb);
        vector<thread> th;
        for (size_t k = 0; k < nb; ++k) {
            clouds[k].reset(new PointCloud());
            th.emplace_back([this, i0, k, &clouds]() { createAndTransformPtCloud((int)(i0 + k), clouds[k]); });
        }
        for (thread& t : th) t.join();
        for (size_t k = 0; k < nb; ++k)
            cloud_big_host.points.insert(cloud_big_host.points.end(), clouds[k]->points.begin(), clouds[k]->points.end());
    }
}

// --preview: the reference's preview thread merges a copy of cloud_big after every cycle (pose.cpp:437-448, 638-674); here
// only the points this cycle appended are folded into the merge kept on the device
void Pose::write_preview(o3dr_ctx* c)
{
    int64_t n_prev = 0;
    uint32_t st = 0;
    chk(o3dr_finalize_incremental(c, nullptr, 0, &n_prev, &st, O3DR_MEM_HOST), "finalize_incremental");
    PointCloud::Ptr prev(new PointCloud());
    prev->points.resize((size_t)(n_prev > 0 ? n_prev : 1));
    chk(o3dr_finalize_incremental(c, prev->points.data(), n_prev > 0 ? n_prev : 1, &n_prev, &st, O3DR_MEM_HOST), "finalize_incremental");
    prev->points.resize((size_t)n_prev);
    string ppath = outputPrefix + "preview.ply";
    save_pt_cloud_to_PLY_File(prev, ppath);
    cout << "preview: " << n_prev << " points" << endl;
}

// The final merge and save (pose.cpp:527-540): cloud.ply and, with --orthophoto_out, the map's rasters
void Pose::merge_and_save(o3dr_ctx* c, PointCloud::Ptr cloud_big_host)
{
    PointCloud::Ptr cloud_small(new PointCloud());
    if (n_gpus > 1 || partitioned_merge) {
        run_sharded(cloud_small);
    } else if (reference_fanout) {
        cloud_small = dont_downsample ? cloud_big_host : downsamplePtCloud(cloud_big_host, true);
    } else {
        int64_t n_big = 0, n_small = 0;
        uint32_t st = 0;
        chk(o3dr_cloud_big_size(c, &n_big, &st), "cloud_big_size");
        cloud_small->points.resize((size_t)(n_big > 0 ? n_big : 1));
        if (!dont_downsample) cout << "downsample before saving..." << endl;
        chk(o3dr_finalize(c, cloud_small->points.data(), n_big > 0 ? n_big : 1, &n_small, &st, O3DR_MEM_HOST), "finalize");
        cloud_small->points.resize((size_t)n_small);
        warn_voxel_overflow(st);
        cout << "cloud_big " << n_big << " points -> cloud " << n_small << " points" << endl;
    }
    cout << "Saving point clouds..." << endl;
    string path = outputPrefix + "cloud.ply";
    save_pt_cloud_to_PLY_File(cloud_small, path);
    if (!orthophoto_out.empty())  // (from the host copy just written: what --orthophoto makes of that cloud.ply)
        write_map_rasters(c, *cloud_small, orthophoto_out + "ortho.png", orthophoto_out + "height.png", orthophoto_out + "shade.png");
}

void Pose::run_reconstruction()
{
    const auto app_start = clk::now();
    o3dr_ctx* c = ctx_for_this_thread();
    chk(o3dr_cloud_big_reset(c), "cloud_big_reset");
    PointCloud::Ptr cloud_big_host(new PointCloud());  // only used by --reference_fanout
    const int n_raw = (int)rawImageDataVec.size(), cycle_len = seq_len > 0 ? seq_len : n_raw;
    acceptedImageDataVec.reserve(rawImageDataVec.size());
    if (!sor && jump_pixels > 0)
        cout << "NOTE: --sor 0: the per-frame StatisticalOutlierRemoval of the reference (pose_functions.cpp:1673-1686) is OFF;\n"
                "      the clouds differ from the reference's for the same command line." << endl;
    const bool sharded_path = n_gpus > 1 || partitioned_merge;
    if (preview && (sharded_path || reference_fanout))
        cout << "--preview: not available on the " << (sharded_path ? "--gpus / --partitioned_merge" : "--reference_fanout")
             << " path" << endl;
    cout << "\n\nProgram Start!" << endl;
    for (int current_idx = 0, cycle = 0; current_idx < n_raw; cycle++) {
        cout << "\nCycle " << cycle << endl;
        const size_t first = acceptedImageDataVec.size();
        accept_cycle(current_idx, cycle_len);
        const size_t last = acceptedImageDataVec.size();
        // ---- point cloud creation for this cycle (pose.cpp:365-434) -------------------------------
        const auto t3 = clk::now();
        cout << "Adding Point Cloud number/points ";
        // (sharded: the frames go to the GPUs as contiguous blocks of the WHOLE accepted list - global frame order is what the
        // merge sums in - so the clouds are made after the last cycle, in run_sharded)
        if (sharded_path) cout << "(deferred: --gpus)";
        else if (reference_fanout) fanout_cycle(first, last, *cloud_big_host);
        else if (last > first) accumulate_cycle(c, first, last);
        chk(o3dr_ctx_synchronize(c), "synchronize");
        const double dt = chrono::duration<double>(clk::now() - t3).count();
        cout << "\n\nPoint Cloud Creation time: " << dt << " sec" << endl;  // pose.cpp:429-431
        if (log_file.is_open()) log_file << "Point Cloud Creation time:\t\t\t" << dt << " sec" << endl;
        if (preview && !sharded_path && !reference_fanout) write_preview(c);
    }
    const double total = chrono::duration<double>(clk::now() - app_start).count();
    cout << "\nFinished Pose Estimation, total time: " << total << " sec at " << acceptedImageDataVec.size() / total << " fps" << endl;
    merge_and_save(c, cloud_big_host);
}

// --gpus N: the fan-out of pose.cpp:392-413 over GPUs instead of threads of one CPU.  Rank g (host thread g, device
// device_id + g) takes the g-th contiguous block of the accepted frames through the batched call; o3dr_merge_partitioned
// then exchanges the per-frame voxels by index slice over RCCL, merges every slice on its GPU and gathers the result.
void Pose::run_sharded(PointCloud::Ptr cloud_small)
{
    const auto t0 = clk::now();
    const size_t n_acc = acceptedImageDataVec.size();
    if (n_gpus < 1) throw runtime_error("--gpus must be at least 1");
    if (dont_downsample) throw runtime_error("--gpus / --partitioned_merge need the downsampling path (no --dont_downsample)");
    if (n_acc == 0) return;
    const FrameBatch b(acceptedImageDataVec, 0, n_acc);  // (unpinned on every way out, after the contexts and communicators go)
    const int W = n_gpus;
    vector<int32_t> devs((size_t)W);
    for (int g = 0; g < W; ++g) devs[(size_t)g] = device_id + g;
    vector<void*> comms((size_t)W, nullptr);
    chk(o3dr_comm_init_all(W, devs.data(), comms.data()), "o3dr_comm_init_all");
    // an upper bound of the merged cloud: no more cells than points, no more points than grid candidates + keypoints
    o3dr_ctx* c0 = ctx_for_this_thread();
    const int64_t cap = o3dr_max_points(c0, rows, cols) * (int64_t)n_acc + b.kp_off[n_acc] + 1;
    cloud_small->points.resize((size_t)cap);
    vector<string> errors((size_t)W);
    vector<int64_t> n_out((size_t)W, 0), n_total((size_t)W, 0);
    vector<uint32_t> st((size_t)W, 0);
    // Every rank's context exists before any rank starts: a rank without one could never enter the exchange, and its
    // peers would wait for it inside the first collective.  Past this point a failure on one rank is carried through the
    // collectives by o3dr_merge_partitioned itself (every rank returns together).
    vector<o3dr_ctx*> ctxs((size_t)W, nullptr);
    for (int g = 0; g < W; ++g) {
        if (o3dr_ctx_create(devs[(size_t)g], &ctxs[(size_t)g]) != O3DR_OK) {
            const string why = o3dr_last_error();
            for (int k = 0; k < g; ++k) (void)o3dr_ctx_destroy(ctxs[(size_t)k]);
            for (int k = 0; k < W; ++k) (void)o3dr_comm_destroy(comms[(size_t)k]);
            throw runtime_error("GPU " + to_string(devs[(size_t)g]) + ": o3dr_ctx_create: " + why);
        }
    }
    vector<thread> th;
    for (int g = 0; g < W; ++g) {
        th.emplace_back([&, g]() {
            o3dr_ctx* c = ctxs[(size_t)g];
            try {
                push_params(c);
                const size_t base = n_acc / (size_t)W, rem = n_acc % (size_t)W;  // contiguous blocks (dist.shard_range)
                const size_t a = (size_t)g * base + min<size_t>((size_t)g, rem), z = a + base + ((size_t)g < rem ? 1 : 0);
                if (z > a)
                    chk(o3dr_accumulate_frames_kp(c, b.disp.data() + a * b.dsz, (int64_t)b.dsz, cols, b.bgr.data() + a * b.csz, (int64_t)b.csz,
                                                  3 * (int64_t)cols, rows, cols, b.poses.data() + 16 * a, (int32_t)(z - a),
                                                  b.kp_xy.empty() ? nullptr : b.kp_xy.data(), b.kp_xy.empty() ? nullptr : b.kp_off.data() + a,
                                                  O3DR_MEM_HOST),
                        "accumulate_frames");
            } catch (const exception& e) {
                errors[(size_t)g] = e.what();
            }
            // (every rank must enter the collective, also after a failure of its own frames: its cloud is then empty)
            if (c) {
                const int rc = o3dr_merge_partitioned(c, comms[(size_t)g], 1, g == 0 ? cloud_small->points.data() : nullptr, g == 0 ? cap : 0,
                                                      &n_out[(size_t)g], &n_total[(size_t)g], &st[(size_t)g], O3DR_MEM_HOST);
                if (rc != O3DR_OK && errors[(size_t)g].empty()) errors[(size_t)g] = string("o3dr_merge_partitioned: ") + o3dr_last_error();
                (void)o3dr_ctx_destroy(c);
            }
        });
    }
    for (thread& t : th) t.join();
    for (int g = 0; g < W; ++g) (void)o3dr_comm_destroy(comms[(size_t)g]);
    for (int g = 0; g < W; ++g)
        if (!errors[(size_t)g].empty()) throw runtime_error("GPU " + to_string(devs[(size_t)g]) + ": " + errors[(size_t)g]);
    cloud_small->points.resize((size_t)n_out[0]);
    warn_voxel_overflow(st[0]);
    const double dt = chrono::duration<double>(clk::now() - t0).count();
    cout << "\n" << W << " GPU(s): cloud_big " << n_total[0] << " points -> cloud " << n_out[0] << " points, " << dt << " sec" << endl;
}

}  // namespace o3dr_host
