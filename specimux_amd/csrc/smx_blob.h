// smx_blob.h -- the table blob of the host files (smx_host.h) and of the HIP-free plans (smx_inner_plan.h).
#ifndef SMX_BLOB_H
#define SMX_BLOB_H
#include <algorithm>
#include <cstring>
#include <vector>

// Appends a table to a blob that goes to the device in one piece: 16-byte aligned, at least 16 bytes.  Returns its offset.
template <typename T>
size_t blob_add(std::vector<unsigned char> &blob, const std::vector<T> &v) {
    size_t off = (blob.size() + 15) & ~(size_t)15;
    blob.resize(off + std::max<size_t>(v.size() * sizeof(T), 16));
    if (!v.empty()) memcpy(blob.data() + off, v.data(), v.size() * sizeof(T));
    return off;
}

#endif  // SMX_BLOB_H
