// tsat_ensemble_launch.hpp — the launchers of the ensemble roll-outs, declared once: each is defined in the unit that holds its
// kernels (a unit per family, so that no existing kernel is recompiled differently) and called by the host code of the entry
// points (tsat_kernels_ensemble.hip), which owns the buffers.
#pragma once
#include <hip/hip_runtime.h>
#include "tsat_model_filtered.hpp"
#include "tsat_mag_filtered.hpp"
#include "tsat_mag_bias_filtered.hpp"
#include "tsat_model_mag_filtered.hpp"
#include "tsat_model_mag_sun_filtered.hpp"

// pack and roll-out of tsat_tvlqr_ensemble_gg (tsat_kernels_gg.hip)
hipError_t tsat_launch_gg_pack(const double* R, double gm, double* GT, int64_t rows, hipStream_t stream);
hipError_t tsat_launch_ensemble_gg(const tsat::GgEnsArgs<double>& g, int waves, hipStream_t stream);
// roll-out of tsat_pd_ensemble (tsat_kernels_pd.hip)
hipError_t tsat_launch_pd(const tsat::PdArgs<double>& a, int waves, hipStream_t stream);
// pack and roll-outs of the sensed calls (tsat_kernels_sensed.hip)
hipError_t tsat_launch_sensed_pack(const double* sensor, double* SN, int64_t T, int M, int Mp, hipStream_t stream);
hipError_t tsat_launch_sensed_tv(const tsat::SensedTvArgs<double>& a, int waves, hipStream_t stream);
hipError_t tsat_launch_sensed_pd(const tsat::SensedPdArgs<double>& a, int waves, hipStream_t stream);
// roll-outs of the filtered calls (tsat_kernels_filtered.hip)
hipError_t tsat_launch_filtered_tv(const tsat::FilteredTvArgs<double>& a, int waves, hipStream_t stream);
hipError_t tsat_launch_filtered_pd(const tsat::FilteredPdArgs<double>& a, int waves, hipStream_t stream);
// roll-outs of the model-filtered calls (tsat_kernels_model_filtered.hip)
hipError_t tsat_launch_model_filtered_tv(const tsat::ModelFilteredTvArgs<double>& a, int waves, hipStream_t stream);
hipError_t tsat_launch_model_filtered_pd(const tsat::ModelFilteredPdArgs<double>& a, int waves, hipStream_t stream);
// roll-outs of the mag-filtered calls (tsat_kernels_mag_filtered.hip)
hipError_t tsat_launch_mag_filtered_tv(const tsat::MagFilteredTvArgs<double>& a, int waves, hipStream_t stream);
hipError_t tsat_launch_mag_filtered_pd(const tsat::MagFilteredPdArgs<double>& a, int waves, hipStream_t stream);
// roll-outs of the mag-bias-filtered calls (tsat_kernels_mag_bias_filtered.hip)
hipError_t tsat_launch_mag_bias_filtered_tv(const tsat::MagBiasFilteredTvArgs<double>& a, int waves, hipStream_t stream);
hipError_t tsat_launch_mag_bias_filtered_pd(const tsat::MagBiasFilteredPdArgs<double>& a, int waves, hipStream_t stream);
// roll-outs of the model-mag-filtered calls (tsat_kernels_model_mag_filtered.hip)
hipError_t tsat_launch_model_mag_filtered_tv(const tsat::ModelMagFilteredTvArgs<double>& a, int waves, hipStream_t stream);
hipError_t tsat_launch_model_mag_filtered_pd(const tsat::ModelMagFilteredPdArgs<double>& a, int waves, hipStream_t stream);
// roll-outs of the model-mag-sun-filtered calls (tsat_kernels_model_mag_sun_filtered.hip)
hipError_t tsat_launch_model_mag_sun_filtered_tv(const tsat::ModelMagSunFilteredTvArgs<double>& a, int waves, hipStream_t stream);
hipError_t tsat_launch_model_mag_sun_filtered_pd(const tsat::ModelMagSunFilteredPdArgs<double>& a, int waves, hipStream_t stream);
