// rtc_cache_check.cpp -- the host side of the hipRTC code-object cache
// (nori-ray-tracer_amd/csrc/rtc_cache.h) on its own, for the sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread \
//       tools/rtc_cache_check.cpp -o tools/rtc_cache_check && tools/rtc_cache_check
// Checks the directory rule (created 0700, used only if this uid owns it),
// the ELF validation on whole, cut, empty, foreign and corrupted images
// (every truncation length and every single-byte change of the headers of a
// small image: no read outside the buffer, the answer only ever "absent"),
// and concurrent writers of one file (a unique temporary file each, the
// published file always one writer's whole image).
#include <dirent.h>

#include <cassert>
#include <thread>

#include "../nori-ray-tracer_amd/csrc/rtc_cache.h"

using namespace nori;

#define CHECK(x)                                                             \
    do {                                                                     \
        if (!(x)) {                                                          \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static void put(std::vector<char> &v, size_t off, uint64_t x, int bytes) {
    for (int i = 0; i < bytes; ++i) v[off + i] = (char)(x >> (8 * i));
}
// A minimal ELF64 image: header, `payload` bytes of one PROGBITS section, a
// NOBITS section larger than the file, the section header table at the end.
static std::vector<char> image(size_t payload, char fill) {
    const size_t shoff = 64 + payload;
    std::vector<char> v(shoff + 3 * 64, 0);
    std::memcpy(v.data(), "\177ELF", 4);
    v[4] = 2;
    v[5] = 1;
    put(v, 0x28, shoff, 8);
    put(v, 0x34, 64, 2);
    put(v, 0x3A, 64, 2);
    put(v, 0x3C, 3, 2);
    for (size_t i = 0; i < payload; ++i) v[64 + i] = fill;
    put(v, shoff + 64 + 4, 1, 4);  // section 1: PROGBITS at 64, `payload` bytes
    put(v, shoff + 64 + 0x18, 64, 8);
    put(v, shoff + 64 + 0x20, payload, 8);
    put(v, shoff + 128 + 4, 8, 4);  // section 2: NOBITS, occupies no file bytes
    put(v, shoff + 128 + 0x18, shoff, 8);
    put(v, shoff + 128 + 0x20, 1u << 20, 8);
    return v;
}
static void spill(const std::string &p, const std::vector<char> &v) {
    FILE *f = std::fopen(p.c_str(), "wb");
    CHECK(f);
    if (!v.empty()) CHECK(std::fwrite(v.data(), 1, v.size(), f) == v.size());
    std::fclose(f);
}
static int count_files(const std::string &d, const char *needle) {
    int n = 0;
    DIR *dir = opendir(d.c_str());
    CHECK(dir);
    while (dirent *e = readdir(dir))
        if (std::strstr(e->d_name, needle)) ++n;
    closedir(dir);
    return n;
}

int main() {
    char tmpl[] = "/tmp/nori_rtc_cache_check.XXXXXX";
    CHECK(mkdtemp(tmpl));
    const std::string root = tmpl, dir = root + "/a/b/cache";

    // ---- the directory: created with its parents, 0700, owned by this uid
    CHECK(!rtc_cache_dir_ok(""));
    CHECK(rtc_cache_dir_ok(dir));
    struct stat st;
    CHECK(stat(dir.c_str(), &st) == 0 && (st.st_mode & 0777) == 0700 && st.st_uid == getuid());
    CHECK(rtc_cache_dir_ok(dir));  // again: it exists
    spill(root + "/file", {});
    CHECK(!rtc_cache_dir_ok(root + "/file"));       // not a directory
    CHECK(!rtc_cache_dir_ok(root + "/file/below"));  // cannot be created
    if (stat("/proc", &st) == 0 && st.st_uid != getuid()) CHECK(!rtc_cache_dir_ok("/proc"));  // another uid's
    setenv("NORI_RTC_CACHE", dir.c_str(), 1);
    CHECK(rtc_cache_dir() == dir);
    setenv("NORI_RTC_CACHE", "0", 1);
    CHECK(rtc_cache_dir().empty());
    unsetenv("NORI_RTC_CACHE");
    setenv("XDG_CACHE_HOME", root.c_str(), 1);
    CHECK(rtc_cache_dir() == root + "/nori_gpu");

    // ---- write, read back, validate
    const std::string file = dir + "/shade_0123456789abcdef.co";
    const std::vector<char> good = image(1000, 'x');
    CHECK(rtc_is_elf(good));
    std::vector<char> got;
    CHECK(!rtc_cache_read(file, got) && got.empty());  // absent
    CHECK(rtc_cache_write(file, good));
    CHECK(rtc_cache_read(file, got) && got == good);
    CHECK(count_files(dir, ".tmp") == 0);
    CHECK(!rtc_cache_write(root + "/missing/x.co", good));  // no directory: nothing written, no throw

    // ---- damaged files are absent: empty, every truncation, no ELF, ELF32, a section past the end
    spill(file, {});
    CHECK(!rtc_cache_read(file, got) && got.empty());
    for (size_t n = 1; n < good.size(); n += (n < 200 || n + 200 > good.size()) ? 1 : 37) {
        const std::vector<char> cut(good.begin(), good.begin() + n);
        CHECK(!rtc_is_elf(cut));
    }
    spill(file, std::vector<char>(good.begin(), good.begin() + good.size() / 2));
    CHECK(!rtc_cache_read(file, got) && got.empty());
    spill(file, std::vector<char>(good.size(), 'X'));
    CHECK(!rtc_cache_read(file, got) && got.empty());
    {
        std::vector<char> v = good;
        v[4] = 1;
        CHECK(!rtc_is_elf(v));
        v = good;
        put(v, 64 + 1000 + 64 + 0x20, 1001 + 3 * 64, 8);  // section 1 one byte past the end
        CHECK(!rtc_is_elf(v));
        v = good;
        put(v, 0x28, ~0ull, 8);  // a section table at 2^64 - 1
        CHECK(!rtc_is_elf(v));
        v = good;
        put(v, 0x3C, 0xFFFF, 2);  // 65535 sections
        CHECK(!rtc_is_elf(v));
    }
    // every single-byte change of the headers: any answer, no read outside the buffer
    {
        const std::vector<char> small = image(8, 'y');
        int ok = 0;
        for (size_t i = 0; i < small.size(); ++i)
            for (int b : {0x00, 0x01, 0x7F, 0x80, 0xFF}) {
                std::vector<char> v = small;
                v[i] = (char)b;
                ok += rtc_is_elf(v) ? 1 : 0;
            }
        std::printf("header bytes changed one at a time: %d of %zu variants still valid\n", ok, small.size() * 5);
    }
    // a damaged file is replaced by the next writer
    CHECK(rtc_cache_write(file, good));
    CHECK(rtc_cache_read(file, got) && got == good);
    rtc_cache_drop(file);
    CHECK(!rtc_cache_read(file, got));
    rtc_cache_drop(file);  // absent: no effect
    rtc_cache_drop("");

    // ---- eight threads write the same file 50 times each, two read: always one writer's whole image
    {
        std::vector<std::thread> ts;
        for (int t = 0; t < 8; ++t)
            ts.emplace_back([&, t] {
                const std::vector<char> mine = image(4096 + 512 * t, (char)('a' + t));
                for (int i = 0; i < 50; ++i) CHECK(rtc_cache_write(file, mine));
            });
        for (int t = 0; t < 2; ++t)
            ts.emplace_back([&] {
                std::vector<char> v;
                for (int i = 0; i < 200; ++i)
                    if (rtc_cache_read(file, v)) {
                        const size_t payload = v.size() - 64 - 3 * 64;
                        CHECK(payload >= 4096 && (payload - 4096) % 512 == 0);
                        const char fill = (char)('a' + (payload - 4096) / 512);
                        for (size_t k = 0; k < payload; ++k) CHECK(v[64 + k] == fill);
                    }
            });
        for (auto &t : ts) t.join();
        CHECK(rtc_cache_read(file, got));
        CHECK(count_files(dir, ".tmp") == 0 && count_files(dir, ".co") == 1);
    }
    const std::string rm = "rm -rf '" + root + "'";
    CHECK(std::system(rm.c_str()) == 0);
    std::puts("rtc_cache_check: ok");
    return 0;
}
