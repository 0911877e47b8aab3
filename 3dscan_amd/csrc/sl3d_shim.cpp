// sl3d_shim.cpp -- drop-in for the reference's stage objects 3/4/5/7: same four C++ entry points, same
// global arrays, same input files, but the arithmetic runs in the HIP kernels behind the C ABI.
// See include/sl3d_shim.h.  Plain C++ (no HIP here); links against libsl3d.so.  The file readers and writers and the host thread
// pool are in sl3d_shim_io.h / sl3d_shim_pool.h.
#include "../../include/sl3d_shim.h"

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <new>
#include <string>
#include <strings.h>
#include <sys/stat.h>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/sl3d.h"
#include "sl3d_shim_io.h"

namespace {

using sl3d_pool::parallel_for;

constexpr int W = Camera_imagewidth, H = Camera_imageheight;
const char *kReferenceRoot = "/home/pranav/Desktop/M_tech_project_console";  // 3/wrapped_phase.cpp:39, 7/triangulation.cpp:152

// One scan runs on one GPU (a single context) or, with SL3D_DEVICES=0,1,..., as row stripes on several (sl3d_group_*: one
// context per listed device, stripe order = row order).  Every stage function below walks the parts; a part's results are
// rows [row0, row0 + rows) of the row-major planes the reference's [col][row] globals are filled from.
struct Part {
    sl3d_ctx *ctx;
    int row0, rows;
    int device = 0;
    sl3d_ctx *twin = nullptr;  // deferred mode: the part's PARITY context (SL3D_FLAG_KEEP_STAGES), created the first time a global
                               // beyond the final ones is asked for (sl3d_shim_materialize)
};

struct Shim {
    sl3d_ctx *ctx = nullptr;    // the first part's context (library-wide calls, error texts)
    sl3d_group *group = nullptr;
    std::vector<Part> parts;
    std::string root;
    bool root_set = false;
    bool write_debug = false;
    bool host_transpose = false;  // A/B switch: row-major download + the transposes on the host
    bool binary_clouds = false;   // save_point_cloud(): binary PCD / PLY instead of the reference's ASCII
    // inputs handed over in memory instead of through the reference's files (sl3d_shim_provide_image / _matrix)
    struct MemImage { const uint8_t *data; int width, height, channels; size_t stride; };
    std::map<std::string, MemImage> images;
    std::map<std::string, std::vector<double>> matrices;
    std::vector<uint8_t> default_mask;  // 1 inside the border, built once
    uint8_t *staging = nullptr;         // pinned: the decoded planes of one stage call, back to back (file inputs)
    size_t staging_planes = 0;
    std::vector<std::vector<uint8_t>> decode_scratch;  // one per staging slot: a file's raw pixel array on its way to the slot
    // save_point_cloud()'s buffers, kept between scans (the reference saves a cloud per scan of its 360-degree loop): 1.9 M points
    // are ~190 MB of text + values, and touching that much FRESH memory costs more than filling it -- every first touch of a page
    // is a fault under the process-wide mm lock, which is what kept 32 formatting threads from scaling.  sl3d_shim_reset frees them.
    std::vector<std::string> pcd_rows, ply_rows;
    std::vector<float> cloud_xyz;
    std::vector<uint8_t> cloud_rgb;
    int status = SL3D_OK;
    std::string err;
    // the configuration the context was created with (the scalar globals may change between scans)
    int F = 0, Nv = 0, Nh = 0, fwv = 0, fwh = 0, ncv = 0, nch = 0;
    // ---- which globals the stage functions fill (sl3d_shim_globals) ----
    // SL3D_SHIM_G_ALL: every stage runs its own kernel and fills its globals when it returns (the contexts keep the stage planes).
    // Anything else = DEFERRED: the three phase stages only bring their inputs to the GPU, triangulate() runs the whole scan as ONE
    // launch of the timed fused kernel and fills the globals the mask names.
    // (never set through sl3d_shim_globals: $SL3D_SHIM_GLOBALS = all | final | none | <hex mask> decides -- a relinked main() can be
    // switched to the deferred mode without touching its source)
    // (case-insensitive; anything that is neither a keyword nor a hexadecimal number is reported and means `all`: a typo must not
    // silently switch a relinked main() to "no globals at all")
    unsigned globals_mask = [] {
        const char *e = getenv("SL3D_SHIM_GLOBALS");
        if (!e || !*e || !strcasecmp(e, "all")) return (unsigned)SL3D_SHIM_G_ALL;
        if (!strcasecmp(e, "final")) return (unsigned)SL3D_SHIM_G_FINAL;
        if (!strcasecmp(e, "none")) return (unsigned)SL3D_SHIM_G_NONE;
        char *end = nullptr;
        const unsigned long v = strtoul(e, &end, 16);
        if (end == e || *end != '\0') {
            fprintf(stderr, "sl3d shim: SL3D_SHIM_GLOBALS=%s is neither all | final | none nor a hexadecimal mask: every global is filled (all)\n", e);
            return (unsigned)SL3D_SHIM_G_ALL;
        }
        return (unsigned)v & (unsigned)SL3D_SHIM_G_EVERY;
    }();
    bool ctx_deferred = false;   // the mode the contexts were created in
    bool scan_open = false;      // deferred: a stage call of the current scan has been made (cleared by triangulate())
    bool mask_fresh = false;     // deferred: selected_region of the current scan is on the device
    bool scan_done = false;      // deferred: triangulate() has run; sl3d_shim_materialize may be called
    bool twin_fresh = false;     // deferred: the parity contexts hold the stage planes of the current scan
    double cal[40] = {0};        // the calibration the contexts hold (set again only when a file's numbers change)
    bool cal_valid = false;
    bool deferred() const { return globals_mask != SL3D_SHIM_G_ALL; }
} g;

std::string data_root()
{
    if (g.root_set) return g.root;
    const char *e = getenv("SL3D_DATA_ROOT");
    return e ? std::string(e) : std::string(kReferenceRoot);
}

// SL3D_SHIM_TIMING=1: the phases of save_point_cloud() on stderr (where a scan's wall time goes once the stages take milliseconds)
struct PhaseTimer {
    bool on = getenv("SL3D_SHIM_TIMING") && atoi(getenv("SL3D_SHIM_TIMING")) != 0;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::string line;
    void lap(const char *what)
    {
        if (!on) return;
        const auto t1 = std::chrono::steady_clock::now();
        char b[96];
        snprintf(b, sizeof b, " %s %.1f ms;", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        line += b;
        t0 = t1;
    }
    void print(const char *who) const
    {
        if (on) fprintf(stderr, "[sl3d shim] %s:%s\n", who, line.c_str());
    }
};

// a stage call that fails abandons the deferred scan in progress: the next stage call opens a new one (it waits for whatever is still
// running and brings selected_region up again) instead of taking this scan's state for its own
void abandon_scan() noexcept { g.scan_open = g.mask_fresh = g.scan_done = false; }

bool fail(int code, const std::string &msg)
{
    g.status = code;
    g.err = msg;
    abandon_scan();
    fprintf(stderr, "\nsl3d shim: %s", msg.c_str());  // the reference reports with printf and carries on
    return false;
}

// The exception barrier of the shim's entry points: the reference's stage functions return void and report with printf, so an exception
// stopped here becomes the shim's status (SL3D_E_NOMEM / SL3D_E_INTERNAL: sl3d_shim_status()) and a line on stderr; the scan in
// progress is abandoned (the next stage call starts from a clean state).  Nothing in here throws.
void shim_caught(const char *where) noexcept;
#define SHIM_CATCH(where) catch (...) { shim_caught(where); }

void shim_caught(const char *where) noexcept
{
    int code = SL3D_E_INTERNAL;
    char buf[320];
    try {
        throw;
    } catch (const std::bad_alloc &) {
        code = SL3D_E_NOMEM;
        snprintf(buf, sizeof buf, "%s: out of host memory (std::bad_alloc)", where);
    } catch (const std::exception &e) {
        snprintf(buf, sizeof buf, "%s: internal error: %s", where, e.what());
    } catch (...) {
        snprintf(buf, sizeof buf, "%s: unknown C++ exception", where);
    }
    g.status = code;
    abandon_scan();
    try {
        g.err = buf;
    } catch (...) {
    }
    fprintf(stderr, "\nsl3d shim: %s", buf);
}

// the status of a libsl3d call: a failure is reported with the status' text and the error text of the context the call was made on
// (NULL: the text the creating calls leave behind)
bool ok(int rc, const char *what, const sl3d_ctx *ctx)
{
    if (rc == SL3D_OK) return true;
    return fail(rc, std::string(what) + ": " + sl3d_strerror(rc) + ": " + sl3d_last_error(ctx));
}

// which context of a part a walk visits: the one the stage calls drive or its parity twin (Part::twin)
enum Side { TIMED, TWIN };

// fn(context, part) for every part in turn; stops at the first failure, reported with the visited context's error text
template <typename Fn>
bool each_part(const char *what, Fn fn, Side side = TIMED)
{
    for (const Part &p : g.parts) {
        sl3d_ctx *c = side == TWIN ? p.twin : p.ctx;
        if (!ok(fn(c, p), what, c)) return false;
    }
    return true;
}

bool sync_parts()
{
    return each_part("sl3d_synchronize", [&](sl3d_ctx *c, const Part &) { return sl3d_synchronize(c); });
}

// One axis of the scan (pattern_type 0 / 1): the reference's four globals of it, their SL3D_G_* ids, its directory name and the number
// of its Gray planes.  The stage functions and fill_globals read the globals from here.
struct Axis {
    int (*&valid)[Camera_imageheight];
    float (*&wrapped)[Camera_imageheight];
    float (*&unwrapped)[Camera_imageheight];
    int (*&code)[Camera_imageheight];
    int id_valid, id_wrapped, id_unwrapped, id_code;
    const char *dir;
    const int &n_gray;
};
const Axis kAxis[2] = {
    {valid_map_vertical, wrapped_phi_vertical, unwrapped_phi_vertical, code_vertical,
     SL3D_G_VALID_V, SL3D_G_WRAPPED_V, SL3D_G_UNWRAPPED_V, SL3D_G_CODE_V, "Vertical", number_of_patterns_binary_vertical},
    {valid_map_horizontal, wrapped_phi_horizontal, unwrapped_phi_horizontal, code_horizontal,
     SL3D_G_VALID_H, SL3D_G_WRAPPED_H, SL3D_G_UNWRAPPED_H, SL3D_G_CODE_H, "Horizontal", number_of_patterns_binary_horizontal},
};
// sl3d_shim_globals names a plane global by the bit of its id
static_assert(SL3D_SHIM_G_VALID_V == 1u << SL3D_G_VALID_V && SL3D_SHIM_G_VALID_H == 1u << SL3D_G_VALID_H && SL3D_SHIM_G_VALID == 1u << SL3D_G_VALID &&
              SL3D_SHIM_G_WRAPPED_V == 1u << SL3D_G_WRAPPED_V && SL3D_SHIM_G_WRAPPED_H == 1u << SL3D_G_WRAPPED_H &&
              SL3D_SHIM_G_UNWRAPPED_V == 1u << SL3D_G_UNWRAPPED_V && SL3D_SHIM_G_UNWRAPPED_H == 1u << SL3D_G_UNWRAPPED_H &&
              SL3D_SHIM_G_CODE_V == 1u << SL3D_G_CODE_V && SL3D_SHIM_G_CODE_H == 1u << SL3D_G_CODE_H, "fill_globals: mask bit = 1 << id");

// One input frame: the caller's memory (sl3d_shim_provide_image under one of the names; no copy) or the first readable file of
// the given names below the data root, decoded into `storage`.
struct Frame {
    const uint8_t *data = nullptr;
    size_t stride = 0;
};

// The input frames of one stage call.  names[i] lists the file names frame i may have (the reference's own and the captured-image
// variant).  A frame provided in memory is used where it lies; all others are decoded from their BMP files ON ALL HOST THREADS AT
// ONCE into one pinned staging area, back to back -- so the files cost one decode time instead of their sum, and the planes go up
// as ONE asynchronous 2-D copy (sl3d_set_frames_range takes back-to-back pinned planes as such).  The staging area is reused by
// the next stage call: every stage function ends with a synchronising getter, so the copy has long finished.
// slot0 / capacity: where in the staging area this call's frames go and how many planes the area must hold -- a stage-by-stage scan
// reuses slots [0, n) in every stage call (after making sure the previous call's copy has finished: an error path may have left it
// in flight); a deferred scan gives every plane of the scan its own slot, so that no stage call waits for the one before it.
bool load_frames(const std::vector<std::vector<std::string>> &names, std::vector<Frame> &out, size_t slot0 = 0, size_t capacity = 0)
{
    const size_t n = names.size();
    if (capacity < slot0 + n) capacity = slot0 + n;
    out.assign(n, Frame());
    std::vector<int> from_file;
    for (size_t i = 0; i < n; i++) {
        for (const auto &nm : names[i]) {
            auto it = g.images.find(nm);
            if (it == g.images.end()) continue;
            const Shim::MemImage &m = it->second;
            if (m.width != W || m.height != H || m.channels != 1) return fail(SL3D_E_INVALID_ARG, "provided image " + nm + " is not an 8-bit gray image of the camera size");
            out[i].data = m.data;
            out[i].stride = m.stride;
            break;
        }
        if (!out[i].data) from_file.push_back((int)i);
    }
    if (from_file.empty()) return true;
    // no asynchronous copy out of the staging area may still be running when it is overwritten or freed
    if ((g.staging_planes < capacity || !g.ctx_deferred) && !sync_parts()) return false;
    if (g.staging_planes < capacity) {
        if (g.staging) sl3d_host_free(g.staging);
        g.staging = (uint8_t *)sl3d_host_alloc(capacity * (size_t)W * H);
        g.staging_planes = g.staging ? capacity : 0;
        if (!g.staging) return fail(SL3D_E_NOMEM, "cannot allocate the pinned staging area for the input frames");
    }
    if (g.decode_scratch.size() < capacity) g.decode_scratch.resize(capacity);
    std::vector<char> ok_flag(n, 1);
    const std::string root = data_root();
    parallel_for((int)from_file.size(), [&](int k) {
        const size_t i = (size_t)from_file[(size_t)k];
        uint8_t *dst = g.staging + (slot0 + i) * (size_t)W * H;   // frames that all come from files end up back to back
        bool got = false;
        for (const auto &nm : names[i])
            if (!got && sl3d_io::read_bmp_gray(root + "/" + nm, W, H, dst, &g.decode_scratch[slot0 + i])) got = true;
        ok_flag[i] = got;
        out[i].data = dst;
        out[i].stride = (size_t)W;
    });
    for (size_t i = 0; i < n; i++)
        if (!ok_flag[i]) return fail(SL3D_E_INVALID_ARG, "cannot read " + root + "/" + names[i][0] + " (8/24-bit BMP of " + std::to_string(W) + "x" + std::to_string(H) + ")");
    return true;
}

// the numbers inside <data>...</data> of an OpenCV XML matrix (cvReadByName of 7/triangulation.cpp:152-168,1069-1083)
bool read_xml_matrix(const std::string &rel, int count, double *out)
{
    {
        auto it = g.matrices.find(rel);
        if (it != g.matrices.end()) {
            if ((int)it->second.size() < count) return fail(SL3D_E_INVALID_ARG, "provided matrix " + rel + " is too short");
            memcpy(out, it->second.data(), sizeof(double) * (size_t)count);
            return true;
        }
    }
    const std::string path = data_root() + "/" + rel;
    std::string s;
    if (!sl3d_io::read_text_file(path, s)) return fail(SL3D_E_INVALID_ARG, "cannot read " + path);
    if (!sl3d_io::parse_xml_matrix(s, count, out)) return fail(SL3D_E_INVALID_ARG, "no <data> with " + std::to_string(count) + " numbers in " + path);
    return true;
}

void drop_ctx()
{
    for (Part &p : g.parts)
        if (p.twin) sl3d_destroy(p.twin);
    abandon_scan();
    g.twin_fresh = g.cal_valid = false;
    if (g.group) sl3d_group_destroy(g.group);
    else if (g.ctx) sl3d_destroy(g.ctx);
    g.group = nullptr;
    g.ctx = nullptr;
    g.parts.clear();
}

// the recorded configuration as a context's: the whole frame on device 0, no flags -- a caller sets what differs
sl3d_config recorded_config()
{
    sl3d_config c;
    memset(&c, 0, sizeof c);
    c.width = W; c.height = H; c.proj_width = Projector_imagewidth; c.proj_height = Projector_imageheight;
    c.n_fringe = g.F; c.n_gray_v = g.Nv; c.n_gray_h = g.Nh;
    c.fringe_width_v = g.fwv; c.fringe_width_h = g.fwh;
    c.n_codes_v = g.ncv; c.n_codes_h = g.nch;
    c.max_views = 1;
    return c;
}

bool ensure_ctx()
{
    const bool same = g.ctx && g.F == number_of_patterns_fringe && g.Nv == number_of_patterns_binary_vertical &&
                      g.Nh == number_of_patterns_binary_horizontal && g.fwv == fringe_width_pixels_vertical &&
                      g.fwh == fringe_width_pixels_horizontal && g.ncv == number_of_codes_vertical && g.nch == number_of_codes_horizontal &&
                      g.ctx_deferred == g.deferred();
    if (same) return true;
    drop_ctx();
    g.ctx_deferred = g.deferred();
    g.F = number_of_patterns_fringe;
    g.Nv = number_of_patterns_binary_vertical; g.Nh = number_of_patterns_binary_horizontal;
    g.fwv = fringe_width_pixels_vertical; g.fwh = fringe_width_pixels_horizontal;
    g.ncv = number_of_codes_vertical; g.nch = number_of_codes_horizontal;
    sl3d_config c = recorded_config();
    c.device = getenv("SL3D_DEVICE") ? atoi(getenv("SL3D_DEVICE")) : 0;
    c.flags = g.ctx_deferred ? 0u : (unsigned)SL3D_FLAG_KEEP_STAGES;  // deferred: the timed kernels, no stage planes
    std::vector<int> devs;
    if (const char *e = getenv("SL3D_DEVICES")) {  // "0,1,2,3": one row stripe per listed device (a device may repeat)
        for (const char *q = e; *q;) {
            char *end = nullptr;
            const long d = strtol(q, &end, 10);
            if (end == q) break;
            devs.push_back((int)d);
            q = *end == ',' ? end + 1 : end;
        }
    }
    if (devs.size() > 1) {
        if (!ok(sl3d_group_create(&c, devs.data(), (int)devs.size(), &g.group), "sl3d_group_create", nullptr)) return false;
        for (int i = 0; i < sl3d_group_size(g.group); i++) {
            Part p{nullptr, 0, 0};
            sl3d_group_stripe(g.group, i, &p.row0, &p.rows, &p.device, &p.ctx);
            g.parts.push_back(p);
        }
        g.ctx = g.parts[0].ctx;
        return true;
    }
    if (devs.size() == 1) c.device = devs[0];
    if (!ok(sl3d_create(&c, &g.ctx), "sl3d_create", nullptr)) return false;
    Part whole{g.ctx, 0, H};
    whole.device = c.device;
    g.parts.push_back(whole);
    return true;
}

// planes [first, first + n) of one axis to every part: a part takes its own rows of every plane (a contiguous byte range)
bool upload_planes(const std::vector<Frame> &img, int pattern_type, int first)
{
    return each_part("sl3d_set_frames_range", [&](sl3d_ctx *c, const Part &q) {
        std::vector<const uint8_t *> planes;
        for (auto &f : img) planes.push_back(f.data + (size_t)q.row0 * f.stride);
        // (planes from different sources may have different strides: one call per run of equal strides)
        size_t i = 0;
        while (i < planes.size()) {
            size_t j = i + 1;
            while (j < planes.size() && img[j].stride == img[i].stride) j++;
            const int rc = sl3d_set_frames_range(c, 0, pattern_type, first + (int)i, planes.data() + i, (int)(j - i), img[i].stride);
            if (rc != SL3D_OK) return rc;
            i = j;
        }
        return (int)SL3D_OK;
    });
}

// The reference allocates its globals with new[] inside the stage functions and never frees them (3/wrapped_phase.cpp:410-424,
// 4/phase_unwrap.cpp:282,300,373-376, 5/compute_correspondance.cpp:635,640, 7/triangulation.cpp:1513).  The shim is that callee: it
// allocates each of them ONCE, in pinned memory, so that it arrives as one full-rate DMA.  count: in elements, not rows.
template <typename T>
void ensure_global(T *&p, size_t count)
{
    using E = typename std::remove_all_extents<T>::type;
    if (p) return;
    void *pinned = sl3d_host_alloc(count * sizeof(E));
    p = pinned ? (T *)pinned : (T *)new E[count];
}
template <typename T>
auto flat(T *p) { return (typename std::remove_all_extents<T>::type *)p; }

// one of the reference's [col][row] globals with K values per pixel, from the parts' contexts or their twins: transposed on the
// device, one contiguous copy per part
bool get_colrow(const char *what, int id, void *dst, Side side = TIMED)
{
    return each_part(what, [&](sl3d_ctx *c, const Part &q) { return sl3d_get_global_colrow(c, 0, id, dst, H, q.row0); }, side);
}
// the same for a stage function; with the A/B switch (sl3d_shim_host_transpose): the row-major plane of T from get_rowmajor and a
// strided host pass
template <typename T, int K = 1, typename U, typename GetRowMajor>
bool fetch_global(const char *what, int id, U *dst, GetRowMajor get_rowmajor, const char *what_rowmajor = nullptr)
{
    if (!g.host_transpose) return get_colrow(what, id, dst);
    std::vector<T> tmp((size_t)W * H * K);
    if (!each_part(what_rowmajor ? what_rowmajor : what, [&](sl3d_ctx *c, const Part &q) { return get_rowmajor(c, tmp.data() + (size_t)q.row0 * W * K); })) return false;
    for (int r = 0; r < H; r++)
        for (int c = 0; c < W; c++)
            for (int k = 0; k < K; k++) dst[((size_t)c * H + r) * K + k] = (U)tmp[((size_t)r * W + c) * K + k];
    return true;
}

// selected_region of image_scissor (m_tech_project_console.cpp:146-238) to every part: handed over in its own int [col][row] layout
// and transposed on the device; without one: 1 inside the border
bool upload_mask()
{
    if (selected_region && !g.host_transpose)
        return each_part("sl3d_set_mask_colrow", [&](sl3d_ctx *c, const Part &) { return sl3d_set_mask_colrow(c, 0, &selected_region[0][0]); });
    std::vector<uint8_t> tmp;
    const uint8_t *mask = nullptr;
    if (selected_region) {
        tmp.assign((size_t)W * H, 0);
        for (int r = 0; r < H; r++)
            for (int c = 0; c < W; c++) tmp[(size_t)r * W + c] = selected_region[c][r] == 1;
        mask = tmp.data();
    } else {
        if (g.default_mask.empty()) {
            g.default_mask.assign((size_t)W * H, 0);
            for (int r = 1; r < H - 1; r++) memset(&g.default_mask[(size_t)r * W + 1], 1, (size_t)W - 2);
        }
        mask = g.default_mask.data();
    }
    return each_part("sl3d_set_mask", [&](sl3d_ctx *c, const Part &) { return sl3d_set_mask(c, 0, mask, W); });
}

// the 8 calibration files of read_parameters() / compute_A() as 40 doubles: Kc dc rc tc Kp dp rp tp
bool read_calibration(double cal[40])
{
    return read_xml_matrix("Camera_calibration/Matrices/cam_intrinsic_mat.xml", 9, cal) &&                                 // 7/triangulation.cpp:152
           read_xml_matrix("Camera_calibration/Matrices/cam_distortion_vect.xml", 5, cal + 9) &&                           // :157
           read_xml_matrix("Triangulation/Camera_extrinsic_parametrs/world_to_cam_rot_vect.xml", 3, cal + 14) &&            // :1069
           read_xml_matrix("Triangulation/Camera_extrinsic_parametrs/world_to_cam_trans_vect.xml", 3, cal + 17) &&          // :1074
           read_xml_matrix("Projector_calibration/Matrices/proj_intrinsic_mat.xml", 9, cal + 20) &&                        // :162
           read_xml_matrix("Projector_calibration/Matrices/proj_distortion_vect.xml", 5, cal + 29) &&                      // :167
           read_xml_matrix("Triangulation/Projector_extrinsic_parametrs/world_to_proj_rot_vect.xml", 3, cal + 34) &&        // :1077
           read_xml_matrix("Triangulation/Projector_extrinsic_parametrs/world_to_proj_trans_vect.xml", 3, cal + 37);        // :1082
}
int set_cal(sl3d_ctx *c, const double cal[40])
{
    return sl3d_set_calibration(c, cal, cal + 9, cal + 14, cal + 17, cal + 20, cal + 29, cal + 34, cal + 37);
}

// the names frame i of a capture directory may have: the reference's own and the captured-image variant.  kind: "Fringe_patterns" or
// "Coded_patterns/Gray_coded"; prefix: "" or "inverse_"
std::vector<std::string> capture_names(const char *kind, const Axis &axis, const char *prefix, int i)
{
    const std::string stem = std::string("Captured_patterns/") + kind + "/" + axis.dir + "/Undistorted/" + prefix, n = std::to_string(i);
    return {stem + "Captured_image_" + n + ".bmp", stem + "Gray_captured_image_" + n + ".bmp"};
}

// ---- deferred mode (sl3d_shim_globals) -------------------------------------------------------------------------------------------
// The first stage call of a scan: the previous scan's launch and copies have finished (its triangulate() may have returned without
// waiting), so the staging slots and the device planes are free to be overwritten.
bool open_deferred_scan()
{
    if (g.scan_open) return true;
    if (!sync_parts()) return false;
    g.scan_open = true;
    g.mask_fresh = g.scan_done = g.twin_fresh = false;
    return true;
}
// first staging slot of an axis' planes: [fringe v, gray v, inverse v, fringe h, gray h, inverse h]
size_t axis_slot0(int pattern_type) { return pattern_type == 0 ? 0 : (size_t)(g.F + 2 * g.Nv); }
size_t scan_slots() { return (size_t)(2 * g.F + 2 * g.Nv + 2 * g.Nh); }

// The parity contexts of a deferred scan: same configuration with SL3D_FLAG_KEEP_STAGES, one per part, on the part's GPU.  They take
// the scan's frames and mask from the parts' own device buffers (device-to-device) and run the scan once more through the per-stage
// kernels, which leave every stage plane behind exactly as the reference's stages leave their globals.  Only sl3d_shim_materialize / a globals mask that names a
// stage global ever gets here.
bool run_twins()
{
    if (g.twin_fresh) return true;
    if (!sync_parts()) return false;  // the parts' uploads run on their own streams: they must have landed before they are copied from
    for (Part &q : g.parts) {
        if (!q.twin) {
            sl3d_config c = recorded_config();
            c.height = q.rows; c.full_width = W; c.full_height = H; c.row0 = q.row0;
            c.device = q.device;
            c.flags = SL3D_FLAG_KEEP_STAGES;
            if (!ok(sl3d_create(&c, &q.twin), "sl3d_create (parity context)", nullptr)) return false;
        }
        sl3d_device_buffers b;
        int rc = sl3d_get_device_buffers(q.ctx, &b);
        // the part's 0/1 mask plane as a full-frame mask: frame pixel (gx, gy) = window pixel (gx, gy - row0)
        // (as an integer: for a part below the frame's first rows that address lies in front of the plane -- it is only where row 0
        // WOULD be; sl3d_set_masks reads, and classifies the memory at, the part's own rows)
        const uint8_t *mask0 = (const uint8_t *)((uintptr_t)b.mask + (uintptr_t)((ptrdiff_t)(2 - q.row0) * (ptrdiff_t)b.mask_pitch + 16));
        if (rc == SL3D_OK) rc = sl3d_set_masks(q.twin, 0, 1, mask0, b.mask_pitch, 0);
        for (int a = 0; a < 2 && rc == SL3D_OK; a++) {
            const int n = g.F + 2 * (a == 0 ? g.Nv : g.Nh);
            std::vector<const uint8_t *> planes((size_t)n);
            for (int i = 0; i < n; i++) planes[(size_t)i] = b.frames + (axis_slot0(a) + (size_t)i) * b.plane_stride;
            rc = sl3d_set_frames(q.twin, 0, a, planes.data(), n, b.frame_pitch);
        }
        if (rc == SL3D_OK) rc = set_cal(q.twin, g.cal);
        // the per-stage kernels, in main()'s order: they leave every plane as the reference's stages leave their globals (the wrapped
        // phase of selected pixels the boundary removal drops, the debug images), which one parity-mode launch of the fused kernel does
        // not (it defines the planes on valid pixels only)
        for (int a = 0; a < 2 && rc == SL3D_OK; a++) rc = sl3d_compute_wrapped_phase(q.twin, 0, a);
        for (int a = 0; a < 2 && rc == SL3D_OK; a++) rc = sl3d_unwrap_phase(q.twin, 0, a);
        if (rc == SL3D_OK) rc = sl3d_compute_c_p_map(q.twin, 0);
        if (rc == SL3D_OK) rc = sl3d_triangulate(q.twin, 0);
        if (!ok(rc, "parity stages", q.twin)) return false;
    }
    g.twin_fresh = true;
    return true;
}

// c_p_map is indexed [row*W + col] in the reference too (common_variables.h:15): the row-major plane is the global
static_assert(sizeof(long int) == sizeof(int64_t), "c_p_map is long[ ][2] on LP64");
bool fetch_c_p_map(Side side)
{
    return each_part("sl3d_get_c_p_map", [&](sl3d_ctx *c, const Part &q) { return sl3d_get_c_p_map(c, 0, (int64_t *)c_p_map + 2 * (size_t)q.row0 * W); }, side);
}

// fills the globals `which` names from the finished deferred scan; the stage globals come from the parity contexts
bool fill_globals(unsigned which)
{
    const size_t px = (size_t)W * H;
    const unsigned stage_bits = which & ~(unsigned)(SL3D_SHIM_G_VALID | SL3D_SHIM_G_INTERSECTION_POINTS_F32);
    if (stage_bits && !run_twins()) return false;
    auto plane = [&](auto *&p, int id, Side side) {  // (a plane global nobody asked for counts as filled)
        if (!(which & 1u << id)) return true;
        ensure_global(p, px);
        return get_colrow("sl3d_get_global_colrow", id, p, side);
    };
    if (!plane(valid_map, SL3D_G_VALID, TIMED)) return false;
    if (which & (SL3D_SHIM_G_INTERSECTION_POINTS | SL3D_SHIM_G_INTERSECTION_POINTS_F32)) {
        ensure_global(intersection_points, px * 3);
        const bool exact = (which & SL3D_SHIM_G_INTERSECTION_POINTS) != 0;
        if (!get_colrow("sl3d_get_global_colrow", exact ? SL3D_G_INTERSECTION_POINTS : SL3D_G_POINTS_F64, intersection_points, exact ? TWIN : TIMED)) return false;
    }
    for (const Axis &a : kAxis)
        if (!plane(a.valid, a.id_valid, TWIN) || !plane(a.wrapped, a.id_wrapped, TWIN) || !plane(a.unwrapped, a.id_unwrapped, TWIN) || !plane(a.code, a.id_code, TWIN)) return false;
    if (which & SL3D_SHIM_G_C_P_MAP) {
        ensure_global(c_p_map, (size_t)total_camera_pixels * 2);
        if (!fetch_c_p_map(TWIN)) return false;
    }
    return true;
}

// the stage-3 / stage-4 debug image of an axis (save_wrapped_image, 3/wrapped_phase.cpp:346; save_unwrap_phase_image,
// 4/phase_unwrap.cpp:321-364): where it goes, and fetching it from the parts (or their twins) and writing it
std::string debug_image_path(int stage, const Axis &axis)
{
    if (stage == 3) return data_root() + "/Wrapped_phase_images/" + axis.dir + "/Wrapped_phase_image.bmp";
    std::string lower = axis.dir;
    lower[0] = (char)tolower(lower[0]);
    return data_root() + "/Unwrapped_phase_images/Gray_coded/" + axis.dir + "/Unwrapped_phase_" + lower + ".bmp";
}
bool write_debug_image(int stage, int pattern_type, Side side = TIMED)
{
    std::vector<uint8_t> d((size_t)W * H);
    if (!each_part("sl3d_get_debug_image", [&](sl3d_ctx *c, const Part &q) { return sl3d_get_debug_image(c, 0, stage, pattern_type, d.data() + (size_t)q.row0 * W, W); }, side))
        return false;
    sl3d_io::write_bmp_gray(debug_image_path(stage, kAxis[pattern_type]), d.data(), W, H);
    return true;
}

// the stage-3 / stage-4 debug images of a deferred scan (sl3d_shim_write_debug_images): from the parity contexts
void write_deferred_debug_images()
{
    if (!run_twins()) return;
    for (int pt = 0; pt < 2; pt++)
        for (int stage = 3; stage <= 4; stage++)
            if (!write_debug_image(stage, pt, TWIN)) return;
}

// A cloud's file or files from its points and colours: the PLY and, with pcd_path, the PCD beside it, in the format
// sl3d_shim_cloud_format selects.  The pieces of both files are produced on all host threads; then the two files go out side by side,
// a write() loop each.  (Writers that start on the finished pieces while the rest is still being formatted were measured too: they
// compete with the formatting threads for the container's CPU quota -- 97 against 83 ms per save.)
bool write_cloud_files(const float *xyz, const uint8_t *rgb, int64_t n, const std::string *pcd_path, const std::string &ply_path, PhaseTimer *pt = nullptr)
{
    const std::string pcd_header = sl3d_io::pcd_header(n, g.binary_clouds), ply_header = sl3d_io::ply_header(n, g.binary_clouds);
    sl3d_io::format_cloud(xyz, rgb, n, g.binary_clouds, pcd_path ? &g.pcd_rows : nullptr, &g.ply_rows);
    if (pt) pt->lap("format");
    // (nothing between the writer thread's start and its join can throw: an exception that unwinds through a joinable std::thread is
    // std::terminate, past the entry point's barrier)
    bool pcd_ok = true;
    std::thread pcd_writer;
    if (pcd_path) pcd_writer = std::thread([&] { pcd_ok = sl3d_io::write_pieces(*pcd_path, pcd_header, g.pcd_rows); });
    const bool ply_ok = sl3d_io::write_pieces(ply_path, ply_header, g.ply_rows);
    if (pcd_path) pcd_writer.join();
    if (pt) pt->lap("write pcd + ply");
    if (!pcd_ok) return fail(SL3D_E_INVALID_ARG, "cannot write " + *pcd_path);
    if (!ply_ok) return fail(SL3D_E_INVALID_ARG, "cannot write " + ply_path);
    return true;
}

}  // namespace


extern "C" void sl3d_shim_set_data_root(const char *dir)
try {
    g.root = dir ? dir : "";
    g.root_set = dir != nullptr;
}
SHIM_CATCH("sl3d_shim_set_data_root")
extern "C" void sl3d_shim_write_debug_images(int enable) { g.write_debug = enable != 0; }
extern "C" int sl3d_shim_last_status(void) { return g.status; }
extern "C" const char *sl3d_shim_last_error(void) { return g.err.c_str(); }
extern "C" void sl3d_shim_reset(void)
try {
    drop_ctx();
    std::vector<std::string>().swap(g.pcd_rows);
    std::vector<std::string>().swap(g.ply_rows);
    std::vector<float>().swap(g.cloud_xyz);
    std::vector<uint8_t>().swap(g.cloud_rgb);
    std::vector<std::vector<uint8_t>>().swap(g.decode_scratch);
}
SHIM_CATCH("sl3d_shim_reset")
extern "C" void sl3d_shim_host_transpose(int enable) { g.host_transpose = enable != 0; }
extern "C" void sl3d_shim_globals(unsigned mask)
{
    g.globals_mask = mask == SL3D_SHIM_G_ALL ? (unsigned)SL3D_SHIM_G_ALL : (mask & (unsigned)SL3D_SHIM_G_EVERY);
}
extern "C" int sl3d_shim_materialize(unsigned which)
try {
    g.status = SL3D_OK;
    if (!g.ctx || !g.ctx_deferred || !g.scan_done) {
        fail(SL3D_E_STATE, "sl3d_shim_materialize: no finished deferred scan (sl3d_shim_globals(mask != SL3D_SHIM_G_ALL), then the six stage calls)");
        return g.status;
    }
    if ((which & (unsigned)SL3D_SHIM_G_EVERY) == 0) sync_parts();  // nothing to fill: only wait until the scan's launch has finished
    else fill_globals(which & (unsigned)SL3D_SHIM_G_EVERY);
    return g.status;
}
catch (...) { shim_caught("sl3d_shim_materialize"); return g.status; }
extern "C" void sl3d_shim_cloud_format(int binary) { g.binary_clouds = binary != 0; }
extern "C" void sl3d_shim_provide_image(const char *relative_path, const uint8_t *data, int width, int height, int channels, size_t stride)
try {
    if (!relative_path) return;
    if (!data) g.images.erase(relative_path);
    else g.images[relative_path] = Shim::MemImage{data, width, height, channels, stride};
}
SHIM_CATCH("sl3d_shim_provide_image")
extern "C" void sl3d_shim_provide_matrix(const char *relative_path, const double *values, int count)
try {
    if (!relative_path) return;
    if (!values) g.matrices.erase(relative_path);
    else g.matrices[relative_path] = std::vector<double>(values, values + count);
}
SHIM_CATCH("sl3d_shim_provide_matrix")

// ---- stage 1: generate_pattern() ----------------------------------------------------------------------
// 1/pattern_generator.cpp:513-544.  The reference's allocate_memory() asks for the number of fringe patterns and the two
// fringe widths with scanf (:204-222); the shim takes them from the globals number_of_patterns_fringe and
// fringe_width_pixels_{vertical,horizontal}, derives number_of_codes_* / number_of_patterns_binary_* exactly as
// :224-229 does (and stores them in the globals, as the reference does), generates every pattern on the device and
// saves the same files save_pattern_images() writes (:414-470) below <data root>/Generated_patterns/.
void generate_pattern()
try {
    g.status = SL3D_OK;
    if (number_of_patterns_fringe < 3 || number_of_patterns_fringe > 5) { fail(SL3D_E_INVALID_ARG, "generate_pattern: 3, 4 or 5 fringe patterns"); return; }
    if (!ok(sl3d_pattern_counts(Projector_imagewidth, fringe_width_pixels_vertical, &number_of_codes_vertical, &number_of_patterns_binary_vertical), "sl3d_pattern_counts", g.ctx)) return;
    if (!ok(sl3d_pattern_counts(Projector_imageheight, fringe_width_pixels_horizontal, &number_of_codes_horizontal, &number_of_patterns_binary_horizontal), "sl3d_pattern_counts", g.ctx)) return;
    if (!ensure_ctx()) return;
    const int PWs = Projector_imagewidth, PHs = Projector_imageheight;
    std::vector<uint8_t> img((size_t)PWs * PHs);
    const std::string root = data_root() + "/Generated_patterns";
    auto emit = [&](int kind, int axis, int index, const std::string &rel) {
        if (!ok(sl3d_generate_pattern(g.ctx, kind, axis, index, img.data(), (size_t)PWs, nullptr, nullptr), "sl3d_generate_pattern", g.ctx)) return false;
        const std::string path = root + "/" + rel;
        const std::string dir = path.substr(0, path.rfind('/'));
        for (size_t i = 1; i <= dir.size(); i++)
            if (i == dir.size() || dir[i] == '/') mkdir(dir.substr(0, i).c_str(), 0777);
        if (!sl3d_io::write_bmp_gray(path, img.data(), PWs, PHs)) return fail(SL3D_E_INVALID_ARG, "cannot write " + path);
        return true;
    };
    for (int axis = 0; axis < 2; axis++) {
        const std::string ax = kAxis[axis].dir;
        for (int i = 0; i < number_of_patterns_fringe; i++)  // :419-431
            if (!emit(SL3D_PATTERN_FRINGE, axis, i, "Fringe_patterns/" + ax + "/Pattern_" + std::to_string(i) + ".bmp")) return;
        for (int j = 0; j < kAxis[axis].n_gray + 1; j++) {  // :433-465: one image more than there are bit planes
            if (!emit(SL3D_PATTERN_BINARY, axis, j, "Coded_patterns/Binary_coded/" + ax + "/Pattern_" + std::to_string(j) + ".bmp")) return;
            if (!emit(SL3D_PATTERN_GRAY, axis, j, "Coded_patterns/Gray_coded/" + ax + "/Pattern_" + std::to_string(j) + ".bmp")) return;
            if (!emit(SL3D_PATTERN_INVERSE_GRAY, axis, j, "Coded_patterns/Gray_coded/" + ax + "/inverse_Pattern_" + std::to_string(j) + ".bmp")) return;
        }
    }
}
SHIM_CATCH("generate_pattern")

// ---- stage 3 ----------------------------------------------------------------------------------------
void compute_wrapped_phase(int pattern_type)
try {
    g.status = SL3D_OK;
    if (pattern_type != 0 && pattern_type != 1) return;
    if (!ensure_ctx()) return;
    const Axis &axis = kAxis[pattern_type];
    const int F = number_of_patterns_fringe;
    std::vector<Frame> img;
    std::vector<std::vector<std::string>> names((size_t)F);
    // read_image: the F fringe frames of this axis (3/wrapped_phase.cpp:29-58); stage 4 brings the Gray / inverse frames
    for (int i = 0; i < F; i++) names[(size_t)i] = capture_names("Fringe_patterns", axis, "", i);
    if (g.ctx_deferred) {
        // deferred: the mask (once per scan: main() calls image_scissor once, m_tech_project_console.cpp:366) and this axis' fringe
        // frames go to the GPU; nothing is computed and no global is touched until triangulate()
        if (!open_deferred_scan()) return;
        if (!g.mask_fresh) {
            if (!upload_mask()) return;
            g.mask_fresh = true;
        }
        if (!load_frames(names, img, axis_slot0(pattern_type), scan_slots())) return;
        upload_planes(img, pattern_type, 0);
        return;
    }
    ensure_global(axis.valid, (size_t)W * H);
    ensure_global(axis.wrapped, (size_t)W * H);

    if (!upload_mask()) return;  // selected_region (image_scissor, m_tech_project_console.cpp:146-238)
    if (!load_frames(names, img)) return;
    if (!upload_planes(img, pattern_type, 0)) return;
    if (!each_part("sl3d_compute_wrapped_phase", [&](sl3d_ctx *c, const Part &) { return sl3d_compute_wrapped_phase(c, 0, pattern_type); })) return;

    if (!fetch_global<uint8_t>("valid map", axis.id_valid, flat(axis.valid), [&](sl3d_ctx *c, uint8_t *d) { return sl3d_get_valid_map(c, 0, pattern_type, d, W); })) return;
    if (!fetch_global<float>("wrapped phase", axis.id_wrapped, flat(axis.wrapped), [&](sl3d_ctx *c, float *d) { return sl3d_get_wrapped_phase(c, 0, pattern_type, d, W); })) return;
    if (g.write_debug) write_debug_image(3, pattern_type);
}
SHIM_CATCH("compute_wrapped_phase")

// ---- stage 4 ----------------------------------------------------------------------------------------
void unwrap_phase(int pattern_type)
try {
    g.status = SL3D_OK;
    if (pattern_type != 0 && pattern_type != 1) return;
    if (!g.ctx) { fail(SL3D_E_STATE, "unwrap_phase before compute_wrapped_phase"); return; }
    if (g.ctx_deferred && !open_deferred_scan()) return;
    const Axis &axis = kAxis[pattern_type];
    if (!g.ctx_deferred) {
        ensure_global(axis.code, (size_t)W * H);
        ensure_global(axis.unwrapped, (size_t)W * H);
    }

    // read_captured_images :51-131: N Gray + N inverse-Gray frames (frame index N is loaded there but never used); the fringe
    // frames of the axis are resident since stage 3
    const int F = number_of_patterns_fringe, N = axis.n_gray;
    std::vector<Frame> img;
    std::vector<std::vector<std::string>> names((size_t)(2 * N));
    for (int i = 0; i < N; i++) {
        names[(size_t)i] = capture_names("Coded_patterns/Gray_coded", axis, "", i);
        names[(size_t)(N + i)] = capture_names("Coded_patterns/Gray_coded", axis, "inverse_", i);
    }
    if (g.ctx_deferred) {  // deferred: the Gray / inverse frames of this axis go to the GPU, nothing else happens here
        if (!load_frames(names, img, axis_slot0(pattern_type) + (size_t)F, scan_slots())) return;
        if (N > 0) upload_planes(img, pattern_type, F);
        return;
    }
    if (!load_frames(names, img)) return;
    if (N > 0 && !upload_planes(img, pattern_type, F)) return;
    if (!each_part("sl3d_unwrap_phase", [&](sl3d_ctx *c, const Part &) { return sl3d_unwrap_phase(c, 0, pattern_type); })) return;

    if (!fetch_global<int32_t>("code", axis.id_code, flat(axis.code), [&](sl3d_ctx *c, int32_t *d) { return sl3d_get_code(c, 0, pattern_type, d, W); })) return;
    if (!fetch_global<float>("unwrapped phase", axis.id_unwrapped, flat(axis.unwrapped), [&](sl3d_ctx *c, float *d) { return sl3d_get_unwrapped_phase(c, 0, pattern_type, d, W); })) return;
    // stage 4 shifts wrapped_phi in place by +Pi (:290, :308)
    if (axis.wrapped && !fetch_global<float>("wrapped phase", axis.id_wrapped, flat(axis.wrapped), [&](sl3d_ctx *c, float *d) { return sl3d_get_wrapped_phase(c, 0, pattern_type, d, W); })) return;
    if (g.write_debug) write_debug_image(4, pattern_type);
}
SHIM_CATCH("unwrap_phase")

// ---- stage 5 ----------------------------------------------------------------------------------------
void compute_c_p_map()
try {
    g.status = SL3D_OK;
    if (!g.ctx) { fail(SL3D_E_STATE, "compute_c_p_map before the phase stages"); return; }
    if (g.ctx_deferred) return;  // deferred: stage 5 is part of triangulate()'s one launch
    ensure_global(valid_map, (size_t)W * H);
    ensure_global(c_p_map, (size_t)total_camera_pixels * 2);
    if (!each_part("sl3d_compute_c_p_map", [&](sl3d_ctx *c, const Part &) { return sl3d_compute_c_p_map(c, 0); })) return;
    if (!fetch_global<uint8_t>("valid map", SL3D_G_VALID, flat(valid_map), [&](sl3d_ctx *c, uint8_t *d) { return sl3d_get_valid_map(c, 0, SL3D_VALID_MERGED, d, W); })) return;
    fetch_c_p_map(TIMED);
}
SHIM_CATCH("compute_c_p_map")

// ---- stage 7 ----------------------------------------------------------------------------------------
void triangulate()
try {
    g.status = SL3D_OK;
    if (!g.ctx) { fail(SL3D_E_STATE, "triangulate before compute_c_p_map"); return; }
    double cal[40];
    if (!read_calibration(cal)) return;
    // (T0 and the per-calibration tables are rebuilt only when a number changed: the reference re-reads the same 8 files every scan)
    if (!g.cal_valid || memcmp(cal, g.cal, sizeof cal) != 0) {
        g.cal_valid = false;
        if (!each_part("sl3d_set_calibration", [&](sl3d_ctx *c, const Part &) { return set_cal(c, cal); })) return;
        memcpy(g.cal, cal, sizeof cal);
        g.cal_valid = true;
    }
    if (g.ctx_deferred) {
        // deferred: stages 3(v) 3(h) 4(v) 4(h) 5 7 as ONE launch of the timed fused kernel on the frames the stage calls brought up
        // (the launch the C ABI's sl3d_run makes: the same kernel bench.py times), then only the globals the mask names
        const bool launched = each_part("sl3d_run", [&](sl3d_ctx *c, const Part &) { return sl3d_run(c, 0, 1); });
        abandon_scan();  // (this scan is over whatever happened: EVERY exit of triangulate() leaves no scan open)
        if (!launched) return;
        g.scan_done = true;
        if (g.globals_mask && !fill_globals(g.globals_mask)) return;
        if (g.write_debug) write_deferred_debug_images();
        return;
    }
    ensure_global(intersection_points, (size_t)W * H * 3);
    if (!each_part("sl3d_triangulate", [&](sl3d_ctx *c, const Part &) { return sl3d_triangulate(c, 0); })) return;
    fetch_global<double, 3>("sl3d_get_global_colrow", SL3D_G_INTERSECTION_POINTS, flat(intersection_points),
                            [&](sl3d_ctx *c, double *d) { return sl3d_get_intersection_points(c, 0, d); }, "sl3d_get_intersection_points");
}
SHIM_CATCH("triangulate")

// ---- stage 8: save_point_cloud() ------------------------------------------------------------------------
// 8/save_point_cloud.cpp:19-217: the valid pixels in row-major scan order (:85-104) as float xyz with the r,g,b of
// Point_cloud/texture.bmp (:46-52,70-72), saved as Point_cloud/point_cloud_<i>.pcd and .ply.  Compaction and colour gather run
// on the device on the result of the last triangulate().  The reference writes the two files with PCL 1.6
// (pcl::io::savePCDFileASCII / savePLYFile, :211-217: both ASCII); PCL is not available here, so the files are standard PCD v0.7
// (fields x y z rgb, rgb as the packed 0x00RRGGBB integer) and PLY (x y z red green blue) that PCL, MeshLab and CloudCompare
// read -- the same points, colours and order, not PCL's exact text (unpinned).  sl3d_shim_cloud_format(1) writes the BINARY
// flavours of both formats (PCD "DATA binary", PLY "binary_little_endian"): the same values bit for bit, without the
// float -> text -> float round trip, and ~30x faster to write.
void save_point_cloud(unsigned cloud_index)
try {
    g.status = SL3D_OK;
    if (!g.ctx) { fail(SL3D_E_STATE, "save_point_cloud before triangulate"); return; }
    PhaseTimer pt;
    std::vector<uint8_t> tex_store;
    const uint8_t *tex = nullptr;
    size_t tex_stride = (size_t)W * 3;
    {
        auto it = g.images.find("Point_cloud/texture.bmp");
        if (it != g.images.end() && it->second.width == W && it->second.height == H && it->second.channels == 3) {
            tex = it->second.data;
            tex_stride = it->second.stride;
        } else if (sl3d_io::read_bmp_bgr(data_root() + "/Point_cloud/texture.bmp", W, H, tex_store)) {
            tex = tex_store.data();
        } else {
            fail(SL3D_E_INVALID_ARG, "cannot read " + data_root() + "/Point_cloud/texture.bmp (8/24-bit BMP of the camera size)");
            return;
        }
    }
    pt.lap("texture read");
    if (!each_part("sl3d_set_texture", [&](sl3d_ctx *c, const Part &q) { return sl3d_set_texture(c, 0, tex + (size_t)q.row0 * tex_stride, tex_stride); })) return;
    pt.lap("texture upload");
    // the parts' clouds one after the other: stripe order = row order = the scan order of :85-104
    int64_t n = 0;
    std::vector<int64_t> cnt(g.parts.size(), 0);
    size_t k = 0;
    if (!each_part("sl3d_get_cloud_rgb", [&](sl3d_ctx *c, const Part &) { const int rc = sl3d_get_cloud_rgb(c, 0, nullptr, nullptr, 0, &cnt[k]); n += cnt[k++]; return rc; })) return;
    std::vector<float> &xyz = g.cloud_xyz;
    std::vector<uint8_t> &rgb = g.cloud_rgb;
    xyz.resize((size_t)n * 3);
    rgb.resize((size_t)n * 3);
    int64_t off = 0;
    k = 0;
    if (!each_part("sl3d_get_cloud_rgb", [&](sl3d_ctx *c, const Part &) {
            int64_t m = 0;
            const int rc = sl3d_get_cloud_rgb(c, 0, xyz.data() + 3 * off, rgb.data() + 3 * off, cnt[k], &m);
            off += cnt[k++];
            return rc;
        }))
        return;
    pt.lap("compaction + download");
    mkdir((data_root() + "/Point_cloud").c_str(), 0777);
    const std::string base = data_root() + "/Point_cloud/point_cloud_" + std::to_string(cloud_index), pcd_path = base + ".pcd", ply_path = base + ".ply";
    const bool written = write_cloud_files(xyz.data(), rgb.data(), n, &pcd_path, ply_path, &pt);
    pt.print("save_point_cloud");
    if (written) fprintf(stderr, "Saved %lld data points to %s.pcd / .ply\n", (long long)n, base.c_str());
}
SHIM_CATCH("save_point_cloud")


// ---- stage 9: register_point_clouds() -------------------------------------------------------------------
// 9/register_point_clouds.cpp:23-155: Point_cloud/point_cloud_<i>.ply, i = 0..n-1, each rotated about the Y axis through
// (tx,ty,tz) by theta_i (theta_0 = 0, theta_{i+1} = theta_i + rot_step in float, degrees with Pi = 22/7), colours kept,
// concatenated into Point_cloud/registered_point_cloud.ply.  Reads the PLY files save_point_cloud() writes, ASCII or binary (vertex
// properties x y z [red green blue] in any order, other properties ignored); the rotation runs on the device.
void register_point_clouds(unsigned num_point_clouds, float tx, float ty, float tz, float rot_step)
try {
    g.status = SL3D_OK;
    if (!ensure_ctx()) return;
    std::vector<float> all_xyz;
    std::vector<uint8_t> all_rgb;
    float theta = 0.0;  // :79
    for (unsigned i = 0; i < num_point_clouds; i++) {
        sl3d_io::PlyCloud c;
        const std::string path = data_root() + "/Point_cloud/point_cloud_" + std::to_string(i) + ".ply";
        if (!sl3d_io::read_ply(path, c)) { fail(SL3D_E_INVALID_ARG, "cannot read " + path + " (ASCII or binary_little_endian PLY with x y z vertex properties)"); return; }
        const int64_t n = (int64_t)c.xyz.size() / 3;
        std::vector<float> out((size_t)n * 3);
        if (!ok(sl3d_transform_cloud(g.ctx, c.xyz.data(), n, theta, tx, ty, tz, out.data()), "sl3d_transform_cloud", g.ctx)) return;
        all_xyz.insert(all_xyz.end(), out.begin(), out.end());
        all_rgb.insert(all_rgb.end(), c.rgb.begin(), c.rgb.end());
        theta += rot_step;  // :145
    }
    write_cloud_files(all_xyz.data(), all_rgb.data(), (int64_t)all_xyz.size() / 3, nullptr, data_root() + "/Point_cloud/registered_point_cloud.ply");
}
SHIM_CATCH("register_point_clouds")
