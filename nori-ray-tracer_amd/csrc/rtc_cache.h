// rtc_cache.h -- the on-disk cache of hipRTC code objects (rtc.hip): where it
// lives, who may use it, and how a file is read, checked and written.  Host
// C++ without HIP, so that tools/rtc_cache_check.cpp exercises it on its own
// under the sanitizers.
//
// The directory ($NORI_RTC_CACHE, else $XDG_CACHE_HOME/nori_gpu,
// ~/.cache/nori_gpu or /tmp/nori_gpu_rtc-<uid>) is created 0700 and used only
// if it is a directory the current uid owns: the /tmp fallback has a
// predictable name that another user could have created first, and a code
// object read from it runs on the GPU.  A file counts only if it is a
// non-empty ELF image; anything else is treated as absent (the caller
// compiles and replaces it).  Writers go through a temporary file of their
// own (mkstemp: unique per writer, threads of one process included) and
// rename it into place.
#pragma once
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace nori {

inline std::string rtc_cache_dir() {
    if (const char *e = std::getenv("NORI_RTC_CACHE")) return e[0] == '0' && !e[1] ? std::string() : std::string(e);
    if (const char *x = std::getenv("XDG_CACHE_HOME"); x && *x) return std::string(x) + "/nori_gpu";
    if (const char *h = std::getenv("HOME"); h && *h) return std::string(h) + "/.cache/nori_gpu";
    return "/tmp/nori_gpu_rtc-" + std::to_string((unsigned)getuid());
}
// Creates the directory (parents 0755, the directory itself 0700) and says
// whether it may be used: a directory owned by the current uid.
inline bool rtc_cache_dir_ok(const std::string &d) {
    if (d.empty()) return false;
    for (size_t i = 1; i <= d.size(); ++i)
        if (i == d.size() || d[i] == '/') {
            const std::string p = d.substr(0, i);
            if (mkdir(p.c_str(), i == d.size() ? 0700 : 0755) != 0 && errno != EEXIST) return false;
        }
    struct stat st;
    return stat(d.c_str(), &st) == 0 && S_ISDIR(st.st_mode) && st.st_uid == getuid();
}
// A whole 64-bit ELF image: the magic, and the program and section header
// tables and every section's bytes inside the file (a file cut short loses
// its section header table, which stands at the end, or a section's tail).
inline bool rtc_is_elf(const std::vector<char> &v) {
    const size_t n = v.size();
    if (n < 64 || std::memcmp(v.data(), "\177ELF", 4) != 0 || v[4] != 2 /* ELFCLASS64 */) return false;
    auto rd = [&](size_t off, size_t bytes) {  // little-endian field; the caller checked off + bytes <= n
        uint64_t x = 0;
        for (size_t i = 0; i < bytes; ++i) x |= (uint64_t)(unsigned char)v[off + i] << (8 * i);
        return x;
    };
    auto inside = [&](uint64_t off, uint64_t len) { return off <= n && len <= n - off; };
    const uint64_t phoff = rd(0x20, 8), shoff = rd(0x28, 8);
    const uint64_t phentsize = rd(0x36, 2), phnum = rd(0x38, 2), shentsize = rd(0x3A, 2), shnum = rd(0x3C, 2);
    if (shoff == 0 || shnum == 0 || shentsize < 64) return false;
    if (!inside(phoff, phentsize * phnum) || !inside(shoff, shentsize * shnum)) return false;
    for (uint64_t i = 0; i < shnum; ++i) {
        const size_t h = (size_t)(shoff + i * shentsize);
        const uint64_t type = rd(h + 4, 4), off = rd(h + 0x18, 8), len = rd(h + 0x20, 8);
        if (type != 8 /* SHT_NOBITS */ && type != 0 && !inside(off, len)) return false;
    }
    return true;
}
// The whole file, if it is a non-empty ELF image; `out` is empty otherwise.
inline bool rtc_cache_read(const std::string &p, std::vector<char> &out) {
    out.clear();
    FILE *f = std::fopen(p.c_str(), "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize(n > 0 ? (size_t)n : 0);
    const bool ok = n > 0 && std::fread(out.data(), 1, out.size(), f) == out.size() && rtc_is_elf(out);
    std::fclose(f);
    if (!ok) out.clear();
    return ok;
}
inline bool rtc_cache_write(const std::string &p, const std::vector<char> &data) {  // atomic: temp file + rename
    std::string tmp = p + ".tmpXXXXXX";
    const int fd = mkstemp(&tmp[0]);
    if (fd < 0) return false;
    size_t done = 0;
    while (done < data.size()) {
        const ssize_t w = write(fd, data.data() + done, data.size() - done);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) break;
        done += (size_t)w;
    }
    const bool ok = close(fd) == 0 && done == data.size();
    if (!ok || std::rename(tmp.c_str(), p.c_str()) != 0) {
        std::remove(tmp.c_str());
        return false;
    }
    return true;
}
inline void rtc_cache_drop(const std::string &p) {
    if (!p.empty()) std::remove(p.c_str());
}

}  // namespace nori
