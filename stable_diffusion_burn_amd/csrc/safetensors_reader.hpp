// safetensors_reader.hpp -- native reader of .safetensors files (the format every downloadable SD v1.x checkpoint comes in).  Host only, no HIP.
//
// Format: 8 bytes little-endian header length N; N bytes of JSON: one object whose members are
//   "<tensor key>": {"dtype": "F16", "shape": [d0, d1, ..], "data_offsets": [begin, end]}
// and, optionally, "__metadata__": {string: string}; then the data section, which the offsets are relative to.  The file is mapped read-only and the tensors
// are indexed in place (key, dtype, shape, pointer into the mapping); nothing is copied until the engine stages them.  The header is parsed by a small JSON
// walker of its own that accepts exactly what the format allows and checks every length against the mapping: a file that lies about a size is refused
// (SDMI_ERR_WEIGHTS; SDMI_ERR_IO when it cannot be opened or mapped) before anything is read through it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

namespace sdmi {

struct StTensor {
    std::string key;
    std::string dtype;            // as the file spells it: "F32", "F16", "BF16", "F64", "I64", ...
    std::vector<int64_t> shape;
    const unsigned char* data;    // inside the mapping; any alignment
    size_t nbytes;                // = product(shape) * size of dtype (checked)
    size_t count;                 // number of elements
    size_t file_offset;           // of `data` in the file
};

class SafetensorsFile {
public:
    explicit SafetensorsFile(const std::string& path);   // maps the file and indexes every tensor; throws sdmi::Error
    ~SafetensorsFile();
    SafetensorsFile(const SafetensorsFile&) = delete;
    SafetensorsFile& operator=(const SafetensorsFile&) = delete;
    const std::vector<StTensor>& tensors() const { return tensors_; }   // in header order
    const StTensor* find(const std::string& key) const;

    // the header alone: `header` = the n JSON bytes, data_bytes = size of the data section the offsets are checked against.  `base` (may be null) is what
    // StTensor::data is relative to.  What the constructor runs; exposed for the sanitizer driver (tests/san/safetensors_main.cpp).
    static void parse_header(const unsigned char* header, size_t n, size_t data_bytes, const unsigned char* base, size_t base_file_offset,
                             std::vector<StTensor>* out);

private:
    void* map_ = nullptr;
    size_t size_ = 0;
    int fd_ = -1;
    std::vector<StTensor> tensors_;
    std::map<std::string, size_t> index_;
};

// bytes per element of a safetensors dtype; 0 for a name the format does not have
size_t safetensors_dtype_size(const std::string& dtype);

}  // namespace sdmi
