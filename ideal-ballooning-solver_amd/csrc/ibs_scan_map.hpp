// Block -> (line, part) map of the one-wave theta0 scans (k_gamma_scan, k_gamma_scan_lean, k_gamma_scan_chain in ibs_kernels.hip):
// the grid the host launches and what a block reads from its indices.  Plain C++ on both sides, so that the host can walk every
// block of a grid and check the cover (tests/test_scan_map_cpu.py).
//
// Workgroups are dealt round-robin over the 8 XCDs in their linear order, so blocks b and b + 8 share an L2.  The `nparts` blocks
// that scan different theta0 of ONE line are therefore placed 8 apart: lines are taken in chunks of 8, and within a chunk the
// line index runs fastest -- a line's geometry is fetched from HBM once per XCD instead of once per block (speed only).
//
// 3-D form (the rule): x = line within its chunk, y = part, z = chunk.  The linear order of the workgroups is
// x + gx * (y + nparts * z), which for full chunks is the order of the 1-D form below -- and a block reads its place from its
// indices, without a division.  gx = 8, or n_lines where that is less (one chunk: every block lives).  The last chunk of a
// launch with n_lines % 8 != 0 holds 8 - n_lines % 8 columns of blocks without a line: they return at once (ScanBlock::live).
//
// 1-D form (where a 3-D grid does not fit: more than 65,535 chunks or parts): b = chunk * 8 * nparts + part * lines_here + line
// within the chunk, lines_here = min(8, n_lines - 8 * chunk); taken apart with three divisions.  No block is idle.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IBS_SM_HD __host__ __device__
#else
#define IBS_SM_HD
#endif

namespace ibs {

constexpr int kScanChunk = 8;             // lines per chunk = XCDs of the device
constexpr long kScanGridLimit = 65535;    // largest y or z extent of a grid

struct ScanGrid {
  unsigned x, y, z;
  int flat;                               // 1 = the 1-D form (kernel argument map_1d)
  long blocks() const { return (long)x * y * z; }
};

// the grid of a scan of n_lines lines in nparts blocks each (both >= 1)
inline ScanGrid scan_grid(long n_lines, long nparts, long limit = kScanGridLimit) {
  const long chunks = (n_lines + kScanChunk - 1) / kScanChunk;
  if (chunks > limit || nparts > limit) return ScanGrid{(unsigned)(nparts * n_lines), 1u, 1u, 1};
  return ScanGrid{(unsigned)(n_lines < kScanChunk ? n_lines : kScanChunk), (unsigned)nparts, (unsigned)chunks, 0};
}

struct ScanBlock {
  int line, part, nparts;
  bool live;                              // false: a column of the last chunk without a line
};

// 3-D form: (bx, by, bz) = blockIdx, ny = gridDim.y
IBS_SM_HD inline ScanBlock scan_block_3d(int n_lines, unsigned bx, unsigned by, unsigned bz, unsigned ny) {
  ScanBlock s;
  s.line = kScanChunk * (int)bz + (int)bx;
  s.part = (int)by;
  s.nparts = (int)ny;
  s.live = s.line < n_lines;
  return s;
}

// 1-D form: b = blockIdx.x of a grid of nparts * n_lines blocks
IBS_SM_HD inline ScanBlock scan_block_1d(int n_lines, int nparts, unsigned b) {
  ScanBlock s;
  const int per = kScanChunk * nparts;
  const int chunk = (int)(b / (unsigned)per), r = (int)b - chunk * per;
  const int rest = n_lines - chunk * kScanChunk;
  const int lines_here = rest < kScanChunk ? rest : kScanChunk;
  s.line = chunk * kScanChunk + r % lines_here;
  s.part = r / lines_here;
  s.nparts = nparts;
  s.live = s.part < nparts;               // (always: r < lines_here * nparts by the grid size)
  return s;
}

}  // namespace ibs
