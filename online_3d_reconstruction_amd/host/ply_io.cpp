// ply_io.cpp — binary PLY in the layout pcl::io::savePLYFileBinary gives a PointXYZRGB cloud
// (pose_functions.cpp:1628-1632): 15-byte vertices (x,y,z float32 + red,green,blue uchar) followed by one
// 84-byte `camera` element; the same header as the reference's bundled build/cloud.ply.  With normals, the
// PointXYZRGBNormal layout: 31-byte vertices (the same six, then normal_x,normal_y,normal_z,curvature float32).
#include <cstdio>
#include <cstring>
#include <sstream>

#include "o3dr_host.h"

namespace o3dr_host {

bool save_ply_binary(const std::string& path, const PointCloud& cloud, const std::vector<float>* normals)
{
    if (normals && normals->size() != cloud.points.size() * 4) return false;
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    std::ostringstream h;
    h << "ply\nformat binary_little_endian 1.0\ncomment PCL generated\n"
      << "element vertex " << cloud.points.size() << "\n"
      << "property float x\nproperty float y\nproperty float z\n"
      << "property uchar red\nproperty uchar green\nproperty uchar blue\n";
    if (normals)
        h << "property float normal_x\nproperty float normal_y\nproperty float normal_z\nproperty float curvature\n";
    h << "element camera 1\n"
      << "property float view_px\nproperty float view_py\nproperty float view_pz\n"
      << "property float x_axisx\nproperty float x_axisy\nproperty float x_axisz\n"
      << "property float y_axisx\nproperty float y_axisy\nproperty float y_axisz\n"
      << "property float z_axisx\nproperty float z_axisy\nproperty float z_axisz\n"
      << "property float focal\nproperty float scalex\nproperty float scaley\n"
      << "property float centerx\nproperty float centery\n"
      << "property int viewportx\nproperty int viewporty\n"
      << "property float k1\nproperty float k2\nend_header\n";
    const std::string hs = h.str();
    fwrite(hs.data(), 1, hs.size(), f);
    const size_t rec_bytes = normals ? 31 : 15;
    std::vector<uint8_t> buf;
    buf.reserve(cloud.points.size() * rec_bytes);
    for (size_t i = 0; i < cloud.points.size(); ++i) {
        const PointXYZRGB& p = cloud.points[i];
        uint8_t rec[31];
        memcpy(rec, &p.x, 4);
        memcpy(rec + 4, &p.y, 4);
        memcpy(rec + 8, &p.z, 4);
        rec[12] = (uint8_t)(p.rgba >> 16);
        rec[13] = (uint8_t)(p.rgba >> 8);
        rec[14] = (uint8_t)p.rgba;
        if (normals) memcpy(rec + 15, normals->data() + 4 * i, 16);
        buf.insert(buf.end(), rec, rec + rec_bytes);
    }
    if (!buf.empty()) fwrite(buf.data(), 1, buf.size(), f);
    // camera: origin, identity axes, zeros, viewport = (width, height) = (n, 1), k1 = k2 = 0
    float cam[17] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0};
    int32_t vp[2] = {(int32_t)cloud.points.size(), 1};
    float k[2] = {0, 0};
    fwrite(cam, 4, 17, f);
    fwrite(vp, 4, 2, f);
    fwrite(k, 4, 2, f);
    fclose(f);
    return true;
}

bool save_ply_mesh(const std::string& path, const PointCloud& cloud, const std::vector<int32_t>& tris, const std::vector<float>* normals)
{
    if (normals && normals->size() != cloud.points.size() * 3) return false;
    if (tris.size() % 3 != 0) return false;
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    std::ostringstream h;
    h << "ply\nformat binary_little_endian 1.0\ncomment PCL generated\n"
      << "element vertex " << cloud.points.size() << "\n"
      << "property float x\nproperty float y\nproperty float z\n"
      << "property uchar red\nproperty uchar green\nproperty uchar blue\n";
    if (normals) h << "property float nx\nproperty float ny\nproperty float nz\n";
    h << "element face " << tris.size() / 3 << "\n"
      << "property list uchar int vertex_indices\nend_header\n";
    const std::string hs = h.str();
    bool ok = fwrite(hs.data(), 1, hs.size(), f) == hs.size();
    const size_t rec_bytes = normals ? 27 : 15;
    std::vector<uint8_t> buf;
    buf.reserve(cloud.points.size() * rec_bytes + tris.size() / 3 * 13);
    for (size_t i = 0; i < cloud.points.size(); ++i) {
        const PointXYZRGB& p = cloud.points[i];
        uint8_t rec[27];
        memcpy(rec, &p.x, 4);
        memcpy(rec + 4, &p.y, 4);
        memcpy(rec + 8, &p.z, 4);
        rec[12] = (uint8_t)(p.rgba >> 16);
        rec[13] = (uint8_t)(p.rgba >> 8);
        rec[14] = (uint8_t)p.rgba;
        if (normals) memcpy(rec + 15, normals->data() + 3 * i, 12);
        buf.insert(buf.end(), rec, rec + rec_bytes);
    }
    for (size_t t = 0; t < tris.size(); t += 3) {
        uint8_t rec[13];
        rec[0] = 3;
        memcpy(rec + 1, &tris[t], 12);
        buf.insert(buf.end(), rec, rec + 13);
    }
    if (!buf.empty()) ok = ok && fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    return fclose(f) == 0 && ok;
}

// the byte size of a PLY scalar type (0: unknown)
static size_t ply_type_size(const std::string& t)
{
    if (t == "char" || t == "uchar" || t == "int8" || t == "uint8") return 1;
    if (t == "short" || t == "ushort" || t == "int16" || t == "uint16") return 2;
    if (t == "int" || t == "uint" || t == "float" || t == "int32" || t == "uint32" || t == "float32") return 4;
    if (t == "double" || t == "float64") return 8;
    return 0;
}

static double ply_scalar(const std::string& t, const uint8_t* p)
{
    if (t == "float" || t == "float32") { float v; memcpy(&v, p, 4); return v; }
    if (t == "double" || t == "float64") { double v; memcpy(&v, p, 8); return v; }
    if (t == "uchar" || t == "uint8") return p[0];
    if (t == "char" || t == "int8") return (int8_t)p[0];
    if (t == "short" || t == "int16") { int16_t v; memcpy(&v, p, 2); return v; }
    if (t == "ushort" || t == "uint16") { uint16_t v; memcpy(&v, p, 2); return v; }
    if (t == "int" || t == "int32") { int32_t v; memcpy(&v, p, 4); return v; }
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

// Binary little-endian PLYs: x y z red green blue are read BY NAME out of the vertex element, whatever other fixed-size
// scalar properties it has (save_ply_binary's 15- and 31-byte layouts among them); elements before it are skipped.
bool read_ply(const std::string& path, PointCloud& cloud)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::string header;
    int ch;
    while ((ch = fgetc(f)) != EOF) {
        header.push_back((char)ch);
        if (header.size() >= 11 && header.compare(header.size() - 11, 11, "end_header\n") == 0) break;
    }
    std::istringstream hs(header);
    std::string line;
    bool binary_le = false, in_vertex = false, seen_vertex = false, ok = true;
    size_t n = 0, skip = 0, rec = 0, elem_count = 0, elem_rec = 0;
    std::vector<std::pair<std::string, std::string>> props;  // vertex (type, name)
    while (ok && std::getline(hs, line)) {
        std::istringstream ls(line);
        std::string kw;
        ls >> kw;
        if (kw == "format") {
            std::string fmt;
            ls >> fmt;
            binary_le = fmt == "binary_little_endian";
        } else if (kw == "element") {
            if (!seen_vertex) skip += elem_count * elem_rec;  // a fixed-size element before the vertices
            std::string name;
            ls >> name >> elem_count;
            elem_rec = 0;
            in_vertex = name == "vertex";
            if (in_vertex) {
                if (seen_vertex) ok = false;
                seen_vertex = true;
                n = elem_count;
            }
        } else if (kw == "property") {
            std::string type, name;
            ls >> type >> name;
            const size_t sz = ply_type_size(type);
            if (sz == 0) {  // a list or an unknown type: the record size is not fixed
                if (in_vertex || !seen_vertex) ok = false;
                continue;
            }
            elem_rec += sz;
            if (in_vertex) {
                props.emplace_back(type, name);
                rec += sz;
            }
        }
    }
    size_t off[6];
    std::string typ[6];
    const char* want[6] = {"x", "y", "z", "red", "green", "blue"};
    for (int k = 0; k < 6 && ok; ++k) {
        size_t o = 0;
        bool found = false;
        for (const auto& pr : props) {
            if (pr.second == want[k]) {
                off[k] = o, typ[k] = pr.first, found = true;
                break;
            }
            o += ply_type_size(pr.first);
        }
        ok = found;
    }
    if (!ok || !binary_le || !seen_vertex || rec == 0 || (skip && fseek(f, (long)skip, SEEK_CUR) != 0)) {
        fclose(f);
        return false;
    }
    std::vector<uint8_t> buf(n * rec);
    const bool got = n == 0 || fread(buf.data(), rec, n, f) == n;
    fclose(f);
    if (!got) return false;
    cloud.points.resize(n);
    for (size_t i = 0; i < n; ++i) {
        const uint8_t* r = &buf[i * rec];
        PointXYZRGB p;
        p.x = (float)ply_scalar(typ[0], r + off[0]);
        p.y = (float)ply_scalar(typ[1], r + off[1]);
        p.z = (float)ply_scalar(typ[2], r + off[2]);
        const uint32_t cr = (uint8_t)ply_scalar(typ[3], r + off[3]), cg = (uint8_t)ply_scalar(typ[4], r + off[4]),
                       cb = (uint8_t)ply_scalar(typ[5], r + off[5]);
        p.rgba = (255u << 24) | (cr << 16) | (cg << 8) | cb;  // PCL's reader leaves a = 255
        cloud.points[i] = p;
    }
    return true;
}

}  // namespace o3dr_host
