// Check of the shim's file readers and writers (3dscan_amd/csrc/sl3d_shim_io.h) and of its host thread pool (sl3d_shim_pool.h), built
// with -fsanitize=address,undefined by tests/test_shim_io.py.  Readers: well-formed files must parse to the right values; truncated,
// oversized, garbage and lying files must be refused (or parsed) WITHOUT touching memory they do not own, allocating what their headers
// claim, or running into undefined behaviour.  Writers: the BMP header byte for byte, the text rows equal to printf's, the pieces of a
// cloud equal to one pass, files that read back bit for bit.  Pool: an exception in one item reaches the caller and stops nothing else.
// Test infrastructure only.   usage: shim_io_check <scratch directory>   -> exit code 0, "ok <cases>" on stdout
#include <atomic>
#include <cfloat>
#include <cstdio>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "sl3d_shim_io.h"

using namespace sl3d_io;
static int failures = 0, cases = 0;
#define CHECK(cond)                                                             \
    do {                                                                        \
        cases++;                                                                \
        if (!(cond)) { failures++; fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); } \
    } while (0)

static void put(const std::string &path, const std::vector<uint8_t> &b)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (b.size()) fwrite(b.data(), 1, b.size(), f);
    fclose(f);
}
static void put_text(const std::string &path, const std::string &s) { put(path, std::vector<uint8_t>(s.begin(), s.end())); }
static void le32(std::vector<uint8_t> &b, size_t o, uint32_t v) { for (int k = 0; k < 4; k++) b[o + k] = (uint8_t)(v >> (8 * k)); }
static std::vector<uint8_t> get(const std::string &path)
{
    std::vector<uint8_t> b;
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return b;
    for (int ch; (ch = fgetc(f)) != EOF;) b.push_back((uint8_t)ch);
    fclose(f);
    return b;
}
static std::string joined(const std::vector<std::string> &pieces)
{
    std::string all;
    for (const auto &q : pieces) all += q;
    return all;
}

// a well-formed BMP of w x h: 8 bits with a grey ramp palette (value = (x + 2 y) & 255) or 24 bits (B, G, R = x, y, x ^ y)
static std::vector<uint8_t> bmp(int w, int h, int bpp, bool top_down = false, uint32_t ncolors = 0)
{
    const size_t rowbytes = (((size_t)w * bpp + 31) / 32) * 4, pal = bpp == 8 ? 4u * (ncolors ? ncolors : 256u) : 0u, off = 54 + pal;
    std::vector<uint8_t> b(off + rowbytes * h, 0);
    b[0] = 'B'; b[1] = 'M';
    le32(b, 2, (uint32_t)b.size()); le32(b, 10, (uint32_t)off); le32(b, 14, 40); le32(b, 18, (uint32_t)w); le32(b, 22, (uint32_t)(top_down ? -h : h));
    b[26] = 1; b[28] = (uint8_t)bpp; le32(b, 46, ncolors);
    if (bpp == 8)
        for (uint32_t i = 0; i < (ncolors ? ncolors : 256u); i++) b[54 + 4 * i] = b[54 + 4 * i + 1] = b[54 + 4 * i + 2] = (uint8_t)i;
    for (int i = 0; i < h; i++) {
        const int y = top_down ? i : h - 1 - i;
        uint8_t *row = &b[off + (size_t)i * rowbytes];
        for (int x = 0; x < w; x++) {
            if (bpp == 8) row[x] = (uint8_t)((x + 2 * y) & (ncolors ? (int)ncolors - 1 : 255));
            else { row[3 * x] = (uint8_t)x; row[3 * x + 1] = (uint8_t)y; row[3 * x + 2] = (uint8_t)(x ^ y); }
        }
    }
    return b;
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : "/tmp";
    const std::string p = dir + "/case.bin";
    const int W = 37, H = 11;
    std::vector<uint8_t> gray((size_t)W * H), bgr, scratch;
    std::mt19937 rng(7);

    // ---- BMP: well-formed files
    for (int bpp : {8, 24})
        for (bool td : {false, true}) {
            put(p, bmp(W, H, bpp, td));
            CHECK(read_bmp_gray(p, W, H, gray.data(), &scratch));
            bool same = true;
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) same &= gray[(size_t)y * W + x] == (bpp == 8 ? (uint8_t)((x + 2 * y) & 255) : bgr2gray(x, y, x ^ y));
            CHECK(same);
            CHECK(read_bmp_bgr(p, W, H, bgr) && bgr.size() == (size_t)W * H * 3);
            CHECK(bpp == 8 ? bgr[3 * (size_t)(5 * W + 3)] == (uint8_t)(3 + 10) : (bgr[3 * (size_t)(5 * W + 3)] == 3 && bgr[3 * (size_t)(5 * W + 3) + 1] == 5));
        }
    put(p, bmp(W, H, 8, false, 16));  // a short palette
    CHECK(read_bmp_gray(p, W, H, gray.data()) && gray[0] == 0 && gray[(size_t)W + 1] == 3);
    // ---- BMP: every truncation of a well-formed file, wrong sizes, lying headers
    for (int bpp : {8, 24}) {
        const std::vector<uint8_t> good = bmp(W, H, bpp);
        for (size_t n = 0; n < good.size(); n += (n < 1200 ? 1 : 97)) {
            put(p, std::vector<uint8_t>(good.begin(), good.begin() + (long)n));
            CHECK(!read_bmp_gray(p, W, H, gray.data(), &scratch));
            CHECK(!read_bmp_bgr(p, W, H, bgr));
        }
        CHECK(!read_bmp_gray(p, W + 1, H, gray.data()) && !read_bmp_gray(p, W, H - 1, gray.data()));
        std::vector<uint8_t> b = good;
        le32(b, 10, 0xfffffff0u);  // pixel array far behind the file
        put(p, b); CHECK(!read_bmp_gray(p, W, H, gray.data()) && !read_bmp_bgr(p, W, H, bgr));
        b = good; le32(b, 10, 10);  // ... inside the header
        put(p, b); CHECK(!read_bmp_gray(p, W, H, gray.data()) && !read_bmp_bgr(p, W, H, bgr));
        b = good; le32(b, 14, 0x7fffffffu);  // a DIB header that puts the palette beyond the file
        put(p, b); CHECK(!read_bmp_gray(p, W, H, gray.data()) && !read_bmp_bgr(p, W, H, bgr));
        b = good; le32(b, 46, 0x40000000u);  // a billion palette entries
        put(p, b); CHECK(bpp == 24 || (!read_bmp_gray(p, W, H, gray.data()) && !read_bmp_bgr(p, W, H, bgr)));
        b = good; le32(b, 30, 1);  // compressed
        put(p, b); CHECK(!read_bmp_gray(p, W, H, gray.data()));
        b = good; b[28] = 4;  // 4 bits per pixel
        put(p, b); CHECK(!read_bmp_gray(p, W, H, gray.data()) && !read_bmp_bgr(p, W, H, bgr));
    }
    // ---- BMP: garbage of every length up to a few KB, and a good header over garbage
    for (int t = 0; t < 300; t++) {
        std::vector<uint8_t> b(rng() % 3000);
        for (auto &x : b) x = (uint8_t)rng();
        if (t % 3 == 0 && b.size() > 60) { const std::vector<uint8_t> g = bmp(W, H, t % 2 ? 8 : 24); std::copy(g.begin(), g.begin() + 30, b.begin()); }
        put(p, b);
        (void)read_bmp_gray(p, W, H, gray.data(), &scratch);  // any answer; no crash, no sanitizer report
        (void)read_bmp_bgr(p, W, H, bgr);
        cases++;
    }
    CHECK(!read_bmp_gray(dir + "/does_not_exist.bmp", W, H, gray.data()));

    // ---- OpenCV XML matrices
    double m[9];
    CHECK(parse_xml_matrix("<?xml version=\"1.0\"?><opencv_storage><M><rows>3</rows><data>\n 1. 2.5e+00 -3 4 5 6 7 8 9e-1</data></M></opencv_storage>", 9, m) && m[1] == 2.5 && m[8] == 0.9);
    CHECK(!parse_xml_matrix("<data>1 2 3</data>", 4, m));                 // too few numbers
    CHECK(!parse_xml_matrix("<data>1 2 3", 3, m));                        // no closing tag
    CHECK(!parse_xml_matrix("</data> 1 2 3 <data>", 3, m));               // tags in the wrong order
    CHECK(!parse_xml_matrix("<data>1 2</data> 3 4 5", 3, m));             // the numbers behind </data> do not count
    CHECK(!parse_xml_matrix("<data>abc</data>", 1, m) && !parse_xml_matrix("", 1, m) && !parse_xml_matrix("<data></data>", 1, m));
    CHECK(parse_xml_matrix("<data>1e999 nan -inf</data>", 3, m));         // whatever strtod makes of it, but no failure of ours
    for (int t = 0; t < 200; t++) {
        std::string s(rng() % 400, ' ');
        for (auto &ch : s) ch = "<>/data0123456789.e-+ \n"[rng() % 23];
        (void)parse_xml_matrix(s, (int)(rng() % 10), m);
        cases++;
    }
    std::string txt;
    put_text(p, "<data>1 2 3</data>");
    CHECK(read_text_file(p, txt) && txt.size() == 18 && !read_text_file(p, txt, 5) && !read_text_file(dir + "/none.xml", txt));

    // ---- PLY
    PlyCloud c;
    const std::string hdr_a = "ply\nformat ascii 1.0\ncomment x\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n";
    put_text(p, hdr_a + "1 2 3 10 20 30\n4 5 6 40 50 60\n-7.5 8 9e1 255 0 128\n");
    CHECK(read_ply(p, c) && c.xyz.size() == 9 && c.xyz[6] == -7.5f && c.xyz[8] == 90.f && c.rgb[3] == 40 && c.rgb[8] == 128);
    put_text(p, hdr_a + "1 2 3 10 20 30\n4 5 6 40 50\n");                  // rows missing
    CHECK(!read_ply(p, c));
    put_text(p, hdr_a + "1 2 3 1e9 -5 nan\n4 5 6 40 50 60\n1e60 -1e60 9 255 0 128\n");   // colours / coordinates out of range: saturate, no UB
    CHECK(read_ply(p, c) && c.rgb[0] == 255 && c.rgb[1] == 0 && c.rgb[2] == 0 && std::isinf(c.xyz[6]) && c.xyz[6] > 0 && c.xyz[7] < 0);
    for (const char *nv : {"4000000000000", "-3", "99999999999999999999999", "12abc", "1000000"}) {   // vertex counts the file cannot hold
        put_text(p, std::string("ply\nformat ascii 1.0\nelement vertex ") + nv + "\nproperty float x\nproperty float y\nproperty float z\nend_header\n1 2 3\n");
        CHECK(!read_ply(p, c));
        put_text(p, std::string("ply\nformat binary_little_endian 1.0\nelement vertex ") + nv + "\nproperty float x\nproperty float y\nproperty float z\nend_header\n123456789012");
        CHECK(!read_ply(p, c));
    }
    {   // binary, mixed types, and its truncations
        std::string b = "ply\nformat binary_little_endian 1.0\nelement vertex 2\nproperty double x\nproperty float y\nproperty short z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty int extra\nend_header\n";
        const size_t h = b.size();
        for (int v = 0; v < 2; v++) {
            double x = 1.5 + v; float y = -2.f * (v + 1); int16_t z = (int16_t)(-7 - v); uint8_t col[3] = {1, 2, (uint8_t)(3 + v)}; int32_t e = 77;
            b.append((const char *)&x, 8); b.append((const char *)&y, 4); b.append((const char *)&z, 2); b.append((const char *)col, 3); b.append((const char *)&e, 4);
        }
        put_text(p, b);
        CHECK(read_ply(p, c) && c.xyz.size() == 6 && c.xyz[3] == 2.5f && c.xyz[4] == -4.f && c.xyz[5] == -8.f && c.rgb[5] == 4);
        for (size_t n = 0; n < b.size(); n += (n < h ? 3 : 1)) {
            put_text(p, b.substr(0, n));
            CHECK(!read_ply(p, c));
        }
    }
    put_text(p, "ply\nformat binary_little_endian 1.0\nelement vertex 1\nproperty quaternion x\nproperty float y\nproperty float z\nend_header\nxxxxxxxxxxxx");
    CHECK(!read_ply(p, c));                                                  // unknown scalar type
    put_text(p, "ply\nformat ascii 1.0\nelement vertex 1\nproperty float x\nproperty float y\nend_header\n1 2\n");
    CHECK(!read_ply(p, c));                                                  // no z
    {
        std::string many = "ply\nformat ascii 1.0\nelement vertex 1\n";
        for (int i = 0; i < 100; i++) many += "property float p" + std::to_string(i) + "\n";
        put_text(p, many + "end_header\n");
        CHECK(!read_ply(p, c));                                              // more properties than anything of ours writes
    }
    for (int t = 0; t < 300; t++) {
        std::string s = t % 2 ? hdr_a : std::string("ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\nend_header\n");
        const size_t n = rng() % 200;
        for (size_t i = 0; i < n; i++) s.push_back((char)rng());
        if (t % 5 == 0) s = s.substr(rng() % (s.size() + 1));
        put_text(p, s);
        (void)read_ply(p, c);
        cases++;
    }
    CHECK(!read_ply(dir + "/none.ply", c));

    // ---- write_bmp_gray: 37 x 11 (a row of 37 bytes is padded to 40) and 8 x 1
    for (const auto &wh : {std::pair<int, int>{37, 11}, std::pair<int, int>{8, 1}}) {
        const int w = wh.first, h = wh.second;
        std::vector<uint8_t> img((size_t)w * h), back((size_t)w * h, 0);
        for (auto &x : img) x = (uint8_t)rng();
        CHECK(write_bmp_gray(p, img.data(), w, h));
        const std::vector<uint8_t> file = get(p);
        // what cvSaveImage writes for a 1-channel image: "BM", the file size, the pixel array at 14 + 40 + 1024, a 40-byte info header with
        // the width, the height (positive: bottom-up), 1 plane, 8 bits, and zero in every other field (biCompression, biSizeImage, the
        // resolutions, biClrUsed, biClrImportant); then 256 palette entries B = G = R = index, reserved byte 0
        const uint32_t rowbytes = (uint32_t)(w + 3) / 4 * 4;
        std::vector<uint8_t> head(1078, 0);
        head[0] = 'B'; head[1] = 'M';
        le32(head, 2, 1078 + rowbytes * (uint32_t)h); le32(head, 10, 1078); le32(head, 14, 40); le32(head, 18, (uint32_t)w); le32(head, 22, (uint32_t)h);
        head[26] = 1; head[28] = 8;
        for (int i = 0; i < 256; i++) head[54 + 4 * i] = head[54 + 4 * i + 1] = head[54 + 4 * i + 2] = (uint8_t)i;
        CHECK(file.size() == 1078 + (size_t)rowbytes * h && std::equal(head.begin(), head.end(), file.begin()));
        CHECK(read_bmp_gray(p, w, h, back.data()) && back == img);
    }
    CHECK(!write_bmp_gray(dir + "/no_such_directory/x.bmp", gray.data(), W, H));

    // ---- the text rows: random bit patterns (the non-finite ones left out: the project defines no text for them) and the edge values
    // against printf("%.9g"), byte for byte
    std::vector<float> xyz = {0.f, -0.f, 1.401298464e-45f, FLT_MIN, FLT_MAX, 1e-5f, 1e-4f, 999999999.f, 1e9f,
                              -1.401298464e-45f, -FLT_MIN, -FLT_MAX, -1e-5f, -1e-4f, -999999999.f, -1e9f, 1.f, 0.1f};
    while (xyz.size() < 3 * 40000) {
        const uint32_t bits = (uint32_t)rng();
        float v;
        memcpy(&v, &bits, 4);
        if (std::isfinite(v)) xyz.push_back(v);
    }
    const int64_t npts = (int64_t)xyz.size() / 3;
    std::vector<uint8_t> rgb((size_t)npts * 3);
    for (auto &x : rgb) x = (uint8_t)rng();
    rgb[0] = rgb[1] = rgb[2] = 0; rgb[3] = rgb[4] = rgb[5] = 255;
    std::string pcd_all, ply_all, pcd_want, ply_want;
    append_cloud_rows(&pcd_all, &ply_all, xyz.data(), rgb.data(), 0, npts);
    for (int64_t i = 0; i < npts; i++) {
        char row[128];
        const unsigned r = rgb[3 * i], g = rgb[3 * i + 1], b = rgb[3 * i + 2];
        snprintf(row, sizeof row, "%.9g %.9g %.9g %u\n", xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], r << 16 | g << 8 | b);
        pcd_want += row;
        snprintf(row, sizeof row, "%.9g %.9g %.9g %u %u %u\n", xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], r, g, b);
        ply_want += row;
    }
    CHECK(pcd_all == pcd_want);
    CHECK(ply_all == ply_want);
    {   // either file alone, a range that does not start at 0, appended behind what the string holds
        std::string only_pcd = "x", only_ply = "y", first_pcd, first_ply;
        append_cloud_rows(&first_pcd, &first_ply, xyz.data(), rgb.data(), 0, 7);
        append_cloud_rows(&only_pcd, nullptr, xyz.data(), rgb.data(), 7, npts - 7);
        append_cloud_rows(nullptr, &only_ply, xyz.data(), rgb.data(), 7, npts - 7);
        CHECK("x" + pcd_want == "x" + first_pcd + only_pcd.substr(1) && only_pcd[0] == 'x');
        CHECK("y" + ply_want == "y" + first_ply + only_ply.substr(1) && only_ply[0] == 'y');
    }

    // ---- the pieces of a cloud: 40,000 points are three uneven pieces; joined they are the one pass above, on all threads and on one
    CHECK(cloud_pieces(0, 16384) == 1 && cloud_pieces(16384, 16384, 8) == 1 && cloud_pieces(16385, 16384, 8) == 2 && cloud_pieces(1 << 30, 65536, 2) == 8);
    for (int threads : {sl3d_pool::usable_threads(), 1}) {
        std::vector<std::string> pcd_pieces(5, "stale"), ply_pieces;
        format_cloud(xyz.data(), rgb.data(), npts, false, &pcd_pieces, &ply_pieces, threads);
        CHECK(pcd_pieces.size() == 3 && ply_pieces.size() == 3 && pcd_pieces[0].size() != pcd_pieces[1].size());
        CHECK(joined(pcd_pieces) == pcd_want && joined(ply_pieces) == ply_want);
        format_cloud(xyz.data(), rgb.data(), npts, false, nullptr, &ply_pieces, threads);   // the buffers again, one file only
        CHECK(joined(ply_pieces) == ply_want);
        // the binary records: 16 bytes (x y z, 0x00RRGGBB) and 15 bytes (x y z, r g b) per point, little endian
        format_cloud(xyz.data(), rgb.data(), npts, true, &pcd_pieces, &ply_pieces, threads);
        const std::string pcd_bin = joined(pcd_pieces), ply_bin = joined(ply_pieces);
        bool same = pcd_pieces.size() == 1 && pcd_bin.size() == (size_t)npts * 16 && ply_bin.size() == (size_t)npts * 15;
        for (int64_t i = 0; i < npts && same; i++) {
            const uint8_t want[4] = {rgb[3 * i + 2], rgb[3 * i + 1], rgb[3 * i], 0};
            same = !memcmp(&pcd_bin[16 * i], &xyz[3 * i], 12) && !memcmp(&pcd_bin[16 * i + 12], want, 4) &&
                   !memcmp(&ply_bin[15 * i], &xyz[3 * i], 12) && !memcmp(&ply_bin[15 * i + 12], &rgb[3 * i], 3);
        }
        CHECK(same);
    }

    // ---- header + pieces through write_pieces, read back by read_ply: the same floats bit for bit, the same colours
    for (bool binary : {false, true}) {
        std::vector<std::string> ply_pieces;
        format_cloud(xyz.data(), rgb.data(), npts, binary, nullptr, &ply_pieces);
        CHECK(write_pieces(p, ply_header(npts, binary), ply_pieces));
        PlyCloud back;
        CHECK(read_ply(p, back) && back.xyz.size() == xyz.size() && !memcmp(back.xyz.data(), xyz.data(), 4 * xyz.size()) && back.rgb == rgb);
        CHECK(get(p).size() == ply_header(npts, binary).size() + joined(ply_pieces).size());
    }
    CHECK(ply_header(12, false) == "ply\nformat ascii 1.0\ncomment generated by sl3d (3dscan_amd)\nelement vertex 12\nproperty float x\nproperty float y\n"
                                   "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n");
    CHECK(pcd_header(12, true) == "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F U\nCOUNT 1 1 1 1\n"
                                  "WIDTH 12\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS 12\nDATA binary\n");
    CHECK(!write_pieces(dir + "/no_such_directory/x.ply", "h", {}));

    // ---- the pool: one item of a burst throws -- the caller gets the exception, every other item has run, the next burst is whole
    {
        std::vector<std::atomic<int>> ran(64);
        bool caught = false;
        try {
            sl3d_pool::parallel_for(64, [&](int i) { ran[(size_t)i]++; if (i == 13) throw std::runtime_error("item 13"); }, 4);
        } catch (const std::runtime_error &e) {
            caught = std::string(e.what()) == "item 13";
        }
        CHECK(caught);
        bool all = true;
        for (auto &r : ran) all &= r == 1;
        CHECK(all);
        sl3d_pool::parallel_for(64, [&](int i) { ran[(size_t)i]++; }, 4);
        all = true;
        for (auto &r : ran) all &= r == 2;
        CHECK(all);
    }
    remove(p.c_str());
    if (failures) { fprintf(stderr, "%d of %d checks failed\n", failures, cases); return 1; }
    printf("ok %d\n", cases);
    return 0;
}
