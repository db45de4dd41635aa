// values_host.cpp -- host-only restatement of the value maps of Solver::set_matrix_values (values.h, DESIGN.md "Matrix values").
// The solver builds its maps on the device with the code that built its matrices; this is the same rule written down plainly,
// reachable from the ABI without a GPU (hprlp_value_maps_host), and what the GPU tests hold the device maps against.
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "values.h"

namespace hprlp {

static std::vector<int> inverse_permutation(const int *new2old, int len, const char *what) {
    std::vector<int> old2new(static_cast<size_t>(len), -1);
    for (int i = 0; i < len; ++i) {
        const int o = new2old[i];
        if (o < 0 || o >= len || old2new[o] >= 0) throw std::runtime_error(std::string("value maps: ") + what + " is not a permutation");
        old2new[o] = i;
    }
    return old2new;
}

void value_maps_host(int m, int n, const int *rowptr, const int *col, const int *row_new2old, const int *col_new2old, int *mapA,
                     int *mapAT) {
    if (m < 0 || n < 0 || !rowptr || !mapA || !mapAT) throw std::runtime_error("value maps: bad arguments");
    if ((row_new2old == nullptr) != (col_new2old == nullptr)) throw std::runtime_error("value maps: both permutations or neither");
    if (rowptr[0] != 0) throw std::runtime_error("value maps: row pointer array does not start at 0");
    for (int i = 0; i < m; ++i)
        if (rowptr[i + 1] < rowptr[i]) throw std::runtime_error("value maps: row pointer array is not monotone");
    const long nnz = rowptr[m];
    if (nnz > 0 && !col) throw std::runtime_error("value maps: bad arguments");
    for (long k = 0; k < nnz; ++k)
        if (col[k] < 0 || col[k] >= n) throw std::runtime_error("value maps: column index out of range");
    // the internal matrix: entry e is the caller's entry mapA[e], in internal column icol[e]
    std::vector<int> icol(static_cast<size_t>(nnz));
    if (!row_new2old) {
        for (long k = 0; k < nnz; ++k) {
            mapA[k] = static_cast<int>(k);
            icol[k] = col[k];
        }
    } else {
        inverse_permutation(row_new2old, m, "row_new2old");
        const std::vector<int> c_old2new = inverse_permutation(col_new2old, n, "col_new2old");
        long e = 0;
        for (int i = 0; i < m; ++i) {  // row i of P A Q is the caller's row row_new2old[i], its columns renumbered and ascending
            const int o = row_new2old[i];
            const long first = e;
            for (int k = rowptr[o]; k < rowptr[o + 1]; ++k) mapA[e++] = k;
            std::stable_sort(mapA + first, mapA + e, [&](int a, int b) { return c_old2new[col[a]] < c_old2new[col[b]]; });
            for (long q = first; q < e; ++q) icol[q] = c_old2new[col[mapA[q]]];
        }
    }
    // its transpose, stable in row order
    std::vector<long> next(static_cast<size_t>(n) + 1, 0);
    for (long e = 0; e < nnz; ++e) ++next[icol[e] + 1];
    for (int j = 0; j < n; ++j) next[j + 1] += next[j];
    for (long e = 0; e < nnz; ++e) mapAT[next[icol[e]]++] = mapA[e];
}

}  // namespace hprlp
