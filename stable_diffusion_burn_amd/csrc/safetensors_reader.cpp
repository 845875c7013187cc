// safetensors_reader.cpp -- see safetensors_reader.hpp.  A bounds-checked JSON walker over the memory-mapped header.
#include "safetensors_reader.hpp"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>

#include "error.hpp"

namespace sdmi {

namespace {

constexpr size_t kMaxHeader = 100u * 1000u * 1000u;   // the format's own limit on the header length

struct Cur {
    const unsigned char* p;
    const unsigned char* end;
    const unsigned char* base;
};

[[noreturn]] void bad(const Cur& c, const std::string& what) {
    throw Error(SDMI_ERR_WEIGHTS, "safetensors header: " + what + " at byte " + std::to_string((size_t)(c.p - c.base)));
}

void skip_ws(Cur& c) {
    while (c.p < c.end && (*c.p == ' ' || *c.p == '\t' || *c.p == '\n' || *c.p == '\r')) ++c.p;
}

void expect(Cur& c, char ch) {
    skip_ws(c);
    if (c.p >= c.end || *c.p != (unsigned char)ch) bad(c, std::string("expected '") + ch + "'");
    ++c.p;
}

// true: the next token is `ch` (consumed)
bool accept(Cur& c, char ch) {
    skip_ws(c);
    if (c.p < c.end && *c.p == (unsigned char)ch) { ++c.p; return true; }
    return false;
}

unsigned hex4(Cur& c) {
    if (c.end - c.p < 4) bad(c, "truncated \\u escape");
    unsigned v = 0;
    for (int i = 0; i < 4; ++i) {
        const unsigned char h = *c.p++;
        v <<= 4;
        if (h >= '0' && h <= '9') v |= h - '0';
        else if (h >= 'a' && h <= 'f') v |= h - 'a' + 10;
        else if (h >= 'A' && h <= 'F') v |= h - 'A' + 10;
        else { --c.p; bad(c, "bad hex digit in \\u escape"); }
    }
    return v;
}

void put_utf8(std::string& s, unsigned cp) {
    if (cp < 0x80) s += (char)cp;
    else if (cp < 0x800) { s += (char)(0xc0 | (cp >> 6)); s += (char)(0x80 | (cp & 0x3f)); }
    else if (cp < 0x10000) { s += (char)(0xe0 | (cp >> 12)); s += (char)(0x80 | ((cp >> 6) & 0x3f)); s += (char)(0x80 | (cp & 0x3f)); }
    else { s += (char)(0xf0 | (cp >> 18)); s += (char)(0x80 | ((cp >> 12) & 0x3f)); s += (char)(0x80 | ((cp >> 6) & 0x3f)); s += (char)(0x80 | (cp & 0x3f)); }
}

// a JSON string: escapes decoded (\uXXXX and surrogate pairs to UTF-8); raw control characters, unknown escapes and lone surrogates are refused
std::string string(Cur& c) {
    expect(c, '"');
    std::string s;
    for (;;) {
        if (c.p >= c.end) bad(c, "unterminated string");
        const unsigned char ch = *c.p++;
        if (ch == '"') return s;
        if (ch < 0x20) { --c.p; bad(c, "control character in a string"); }
        if (ch != '\\') { s += (char)ch; continue; }
        if (c.p >= c.end) bad(c, "unterminated string");
        const unsigned char e = *c.p++;
        switch (e) {
            case '"': s += '"'; break;
            case '\\': s += '\\'; break;
            case '/': s += '/'; break;
            case 'b': s += '\b'; break;
            case 'f': s += '\f'; break;
            case 'n': s += '\n'; break;
            case 'r': s += '\r'; break;
            case 't': s += '\t'; break;
            case 'u': {
                unsigned cp = hex4(c);
                if (cp >= 0xdc00 && cp <= 0xdfff) bad(c, "lone low surrogate");
                if (cp >= 0xd800 && cp <= 0xdbff) {
                    if (c.end - c.p < 2 || c.p[0] != '\\' || c.p[1] != 'u') bad(c, "lone high surrogate");
                    c.p += 2;
                    const unsigned lo = hex4(c);
                    if (lo < 0xdc00 || lo > 0xdfff) bad(c, "lone high surrogate");
                    cp = 0x10000 + ((cp - 0xd800) << 10) + (lo - 0xdc00);
                }
                put_utf8(s, cp);
                break;
            }
            default: --c.p; bad(c, "unknown escape in a string");
        }
    }
}

// a non-negative JSON integer that fits int64
int64_t integer(Cur& c, const char* what) {
    skip_ws(c);
    if (c.p < c.end && *c.p == '-') bad(c, std::string("negative ") + what);
    if (c.p >= c.end || *c.p < '0' || *c.p > '9') bad(c, std::string("expected an integer for ") + what);
    if (*c.p == '0' && c.end - c.p > 1 && c.p[1] >= '0' && c.p[1] <= '9') bad(c, "leading zero in a number");
    uint64_t v = 0;
    while (c.p < c.end && *c.p >= '0' && *c.p <= '9') {
        const unsigned d = *c.p - '0';
        if (v > ((uint64_t)INT64_MAX - d) / 10) bad(c, std::string(what) + " overflows");
        v = v * 10 + d;
        ++c.p;
    }
    if (c.p < c.end && (*c.p == '.' || *c.p == 'e' || *c.p == 'E')) bad(c, std::string(what) + " is not an integer");
    return (int64_t)v;
}

// "__metadata__": {string: string}; anything nested is not the format
void metadata(Cur& c) {
    expect(c, '{');
    if (accept(c, '}')) return;
    do {
        skip_ws(c);
        (void)string(c);
        expect(c, ':');
        skip_ws(c);
        if (c.p < c.end && (*c.p == '{' || *c.p == '[')) bad(c, "nested value in __metadata__");
        if (c.p >= c.end || *c.p != '"') bad(c, "__metadata__ values must be strings");
        (void)string(c);
    } while (accept(c, ','));
    expect(c, '}');
}

}  // namespace

size_t safetensors_dtype_size(const std::string& d) {
    static const struct { const char* name; size_t size; } k[] = {
        {"BOOL", 1}, {"U8", 1}, {"I8", 1}, {"F8_E5M2", 1}, {"F8_E4M3", 1}, {"I16", 2}, {"U16", 2}, {"F16", 2}, {"BF16", 2},
        {"I32", 4}, {"U32", 4}, {"F32", 4}, {"F64", 8}, {"I64", 8}, {"U64", 8}};
    for (const auto& e : k)
        if (d == e.name) return e.size;
    return 0;
}

void SafetensorsFile::parse_header(const unsigned char* header, size_t n, size_t data_bytes, const unsigned char* base, size_t base_file_offset,
                                   std::vector<StTensor>* out) {
    Cur c{header, header + n, header};
    std::map<std::string, int> seen;
    expect(c, '{');
    if (!accept(c, '}')) {
        do {
            skip_ws(c);
            const Cur at = c;
            std::string key = string(c);
            if (!seen.emplace(key, 0).second) bad(at, "duplicate key '" + key + "'");
            expect(c, ':');
            if (key == "__metadata__") { metadata(c); continue; }
            StTensor t{};
            t.key = std::move(key);
            int64_t begin = -1, end = -1;
            bool have_shape = false;
            expect(c, '{');
            do {
                skip_ws(c);
                const Cur fat = c;
                const std::string field = string(c);
                expect(c, ':');
                if (field == "dtype" && t.dtype.empty()) {
                    skip_ws(c);
                    t.dtype = string(c);
                    if (t.dtype.empty()) bad(fat, "empty dtype");
                } else if (field == "shape" && !have_shape) {
                    have_shape = true;
                    expect(c, '[');
                    if (!accept(c, ']')) {
                        do t.shape.push_back(integer(c, "dimension")); while (accept(c, ','));
                        expect(c, ']');
                    }
                } else if (field == "data_offsets" && begin < 0) {
                    expect(c, '[');
                    begin = integer(c, "offset");
                    expect(c, ',');
                    end = integer(c, "offset");
                    expect(c, ']');
                } else {
                    bad(fat, "unexpected or repeated field '" + field + "' of '" + t.key + "'");
                }
            } while (accept(c, ','));
            expect(c, '}');
            if (t.dtype.empty() || !have_shape || begin < 0) bad(at, "'" + t.key + "' lacks dtype, shape or data_offsets");
            const size_t esz = safetensors_dtype_size(t.dtype);
            if (!esz) bad(at, "'" + t.key + "' has unknown dtype '" + t.dtype + "'");
            if (begin > end) bad(at, "'" + t.key + "': data_offsets are reversed");
            if ((uint64_t)end > (uint64_t)data_bytes) bad(at, "'" + t.key + "': data_offsets [" + std::to_string(begin) + ", " + std::to_string(end) + ") lie outside the data section of " + std::to_string(data_bytes) + " bytes");
            uint64_t count = 1;
            for (int64_t d : t.shape) {
                if (d != 0 && count > (uint64_t)INT64_MAX / (uint64_t)d) bad(at, "'" + t.key + "': the shape's product overflows");
                count *= (uint64_t)d;
            }
            if (count > (uint64_t)INT64_MAX / esz) bad(at, "'" + t.key + "': the shape's product overflows");
            if (count * esz != (uint64_t)(end - begin))
                bad(at, "'" + t.key + "': shape x " + t.dtype + " is " + std::to_string(count * esz) + " bytes, data_offsets span " + std::to_string(end - begin));
            t.count = (size_t)count;
            t.nbytes = (size_t)(end - begin);
            t.file_offset = base_file_offset + (size_t)begin;
            t.data = base ? base + begin : nullptr;
            out->push_back(std::move(t));
        } while (accept(c, ','));
        expect(c, '}');
    }
    skip_ws(c);   // writers pad the header with spaces
    if (c.p != c.end) bad(c, "trailing bytes after the header object");
    // overlap: by begin offset, every tensor ends before the next one starts (empty tensors may share an offset)
    std::vector<const StTensor*> order;
    for (const StTensor& t : *out)
        if (t.nbytes) order.push_back(&t);
    std::sort(order.begin(), order.end(), [](const StTensor* a, const StTensor* b) { return a->file_offset < b->file_offset; });
    for (size_t i = 1; i < order.size(); ++i)
        if (order[i - 1]->file_offset + order[i - 1]->nbytes > order[i]->file_offset)
            throw Error(SDMI_ERR_WEIGHTS, "safetensors header: '" + order[i - 1]->key + "' and '" + order[i]->key + "' overlap");
}

SafetensorsFile::SafetensorsFile(const std::string& path) {
    fd_ = ::open(path.c_str(), O_RDONLY);
    if (fd_ < 0) throw Error(SDMI_ERR_IO, "cannot open " + path);
    struct stat st {};
    if (fstat(fd_, &st) != 0 || !S_ISREG(st.st_mode)) { ::close(fd_); throw Error(SDMI_ERR_IO, "not a regular file: " + path); }
    size_ = (size_t)st.st_size;
    if (size_ < 8) { ::close(fd_); throw Error(SDMI_ERR_WEIGHTS, path + ": shorter than the 8-byte header length of a safetensors file"); }
    map_ = mmap(nullptr, size_, PROT_READ, MAP_PRIVATE, fd_, 0);
    if (map_ == MAP_FAILED) { map_ = nullptr; ::close(fd_); throw Error(SDMI_ERR_IO, "mmap failed: " + path); }
    try {
        const unsigned char* b = static_cast<const unsigned char*>(map_);
        uint64_t hlen = 0;
        for (int i = 7; i >= 0; --i) hlen = (hlen << 8) | b[i];
        if (hlen > kMaxHeader) throw Error(SDMI_ERR_WEIGHTS, path + ": header length " + std::to_string(hlen) + " exceeds the format's 100 MB limit (not a safetensors file?)");
        if (hlen > size_ - 8) throw Error(SDMI_ERR_WEIGHTS, path + ": header length " + std::to_string(hlen) + " exceeds the file's " + std::to_string(size_) + " bytes");
        parse_header(b + 8, (size_t)hlen, size_ - 8 - (size_t)hlen, b + 8 + hlen, 8 + (size_t)hlen, &tensors_);
        for (size_t i = 0; i < tensors_.size(); ++i) index_[tensors_[i].key] = i;
    } catch (const Error& e) {
        munmap(map_, size_);
        ::close(fd_);
        if (e.status == SDMI_ERR_WEIGHTS && std::string(e.what()).compare(0, path.size(), path) != 0) throw Error(SDMI_ERR_WEIGHTS, path + ": " + e.what());
        throw;
    } catch (...) {
        munmap(map_, size_);
        ::close(fd_);
        throw;
    }
}

SafetensorsFile::~SafetensorsFile() {
    if (map_) munmap(map_, size_);
    if (fd_ >= 0) ::close(fd_);
}

const StTensor* SafetensorsFile::find(const std::string& key) const {
    auto it = index_.find(key);
    return it == index_.end() ? nullptr : &tensors_[it->second];
}

}  // namespace sdmi
