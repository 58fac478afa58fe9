// cert_ws.h -- the layout of ctx->cert, the one device workspace the analysis passes share (api_analysis.hip): the results a pass
// copies back, then the per-workgroup records of its reduction; the passes that make their own full pass over the rows keep its
// d-vector grad f(x) (elements of the rows' type) behind the struct.  All doubles; no kernel here.
#pragma once

#include <stddef.h>

namespace ciao {

constexpr int CERT_GRID_CAP = 512;      // cert_kernels.h and what is built as it is: workgroups (= partial records) at most
constexpr int CERT_REC = 8;             // doubles per record: S0 S1 S2 M V + padding to 64 bytes
constexpr int ROWSQ_WG_TARGET = 2048;   // rowsq_kernels.h: workgroups (= records) at most: 8 per CU
constexpr int ROWSQ_REC = 8;            // doubles per record: max, argmax, min, sum + padding to 64 bytes

// launch_cert's five results (cert_kernels.h says what they are) and what the certificate's own pass over the rows leaves behind them
struct CertResults {
    double S0, S1, S2, M, V;
    double unused;
    double obj[2];   // that pass's Epilogue::obj_out: the epilogue writes obj[1], here the RAW sum of the f_i(x)
};

// ciao_certificate
struct CertWs {
    CertResults res;
    double rec[CERT_GRID_CAP * CERT_REC];
};

// ciao_row_dots, ciao_margin_stats, ciao_certificate_samples: the two reductions use the records one after the other
struct MstatWs {
    CertResults res;
    double stat[8];   // [0..4) launch_mstat's four results
    double rec[CERT_GRID_CAP * CERT_REC];
};

// ciao_screen
struct ScreenWs {
    double count;   // the kept coordinates
    double unused[7];
    double rec[CERT_GRID_CAP * CERT_REC];
};

// ciao_row_sqnorms
struct RowsqWs {
    double summary[8];   // [0..4) max, argmax, min, sum
    double rec[ROWSQ_WG_TARGET * ROWSQ_REC];
};

constexpr int CERT_WS_DOUBLES = sizeof(CertWs) / sizeof(double);
constexpr int MSTAT_WS_DOUBLES = sizeof(MstatWs) / sizeof(double);
constexpr int SCREEN_WS_DOUBLES = sizeof(ScreenWs) / sizeof(double);
constexpr int ROWSQ_WS_DOUBLES = sizeof(RowsqWs) / sizeof(double);

// the numbers these names replaced, offset by offset
static_assert(CERT_WS_DOUBLES == 8 + 512 * 8 && MSTAT_WS_DOUBLES == 16 + 512 * 8 && SCREEN_WS_DOUBLES == 8 + 512 * 8 &&
                  ROWSQ_WS_DOUBLES == 8 + 2048 * 8,
              "the allocated sizes");
static_assert(offsetof(CertResults, S0) == 0 && offsetof(CertResults, S1) == 8 && offsetof(CertResults, S2) == 2 * 8 &&
                  offsetof(CertResults, M) == 3 * 8 && offsetof(CertResults, V) == 4 * 8,
              "h[0..5): S0 S1 S2 M V; res + 3: the device-formed dual scaling reads M");
static_assert(offsetof(CertResults, obj) == 6 * 8, "res + 6 = obj_out, read back as h[7]");
static_assert(offsetof(CertWs, rec) == 8 * 8 && offsetof(ScreenWs, rec) == 8 * 8 && offsetof(RowsqWs, rec) == 8 * 8, "res + 8: the records");
static_assert(offsetof(MstatWs, stat) == 8 * 8 && offsetof(MstatWs, rec) == 16 * 8, "res + 8: the four statistics; res + 16: the records");

}  // namespace ciao
