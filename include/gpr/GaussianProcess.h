// gpr/GaussianProcess.h — GaussianProcess<T> host API over libgprx.
//
// Same public surface as the reference class (include/GaussianProcess.h:33-328):
// AddSample, Initialize, Predict, PredictDerivative, operator()(x,y), GetCredibleInterval,
// Get/SetKernel, Get/SetSigma, SetInversionMethod, Get/SetEfficientStorage, Save, Load,
// ToString, Lock/UnLock, operator==.  The numerics are done by libgprx on the GPU: the
// training set, the Cholesky factor of K + sigma^2 I and the regression vectors stay
// resident in HBM; the host keeps the sample lists (for Save / ==) and a copy of the
// regression vectors (m_RegressionVectors, as the reference).
//
// Kernels with no device form (a user Kernel<T> subclass that does not override Describe):
// K, the query kernel vectors and the derivative matrices are evaluated on the host through
// the virtual operator() / GetDerivative, as the reference does for every kernel; the
// factorisation, solves and reductions still run on the device (gprx_model_set_kernel_matrix
// and the *_kx entry points of include/gprx.h).
//
// Differences (documented in DESIGN.md): the core matrix C = (K + sigma^2 I)^{-1} is
// materialised lazily from the device factor (Save, GetCoreMatrix), not at every
// Initialize; operator()/GetCredibleInterval use the factor (k - |L^{-1}k|^2) instead of
// Kx^T C Ky.  InversionMethod (lib/GaussianProcess.cpp:531-618): FullPivotLU (default) and
// SelfAdjointEigenSolver factorise with Cholesky and, when K + sigma^2 I is not numerically
// positive definite, fall back to a partial-pivot LU in double (FullPivotLU = dgetrf_,
// include/LAPACKUtils.h:38-56; gpr_amd/csrc/k_getrf.hip); JacobiSVD / BDCSVD, whose formula is
// the exact inverse V S^{-1} U^T, factorise with that LU directly (no SVD is formed).
//
// Threading (reference: tests/PosteriorProcessTest.cpp:120-134 calls Predict and operator()
// concurrently after Initialize): the read-only calls may run concurrently; the lazy device
// refit behind operator()/GetCoreMatrix after Load is guarded by m_DevMu, and libgprx
// serialises the device calls of one context.
#pragma once

#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../gprx.h"
#include "Kernel.h"
#include "Matrix.h"

namespace gpr {

template <class T>
class Likelihood;
template <class T>
class GaussianLogLikelihood;
template <class T>
class GaussianLikelihood;

// Process-wide libgprx context (device from $GPRX_DEVICE, default 0).  Throws std::string
// when no GPU is visible: there is no CPU fallback.
gprx_ctx* DefaultContext();
// Throw the reference-style std::string for a failed libgprx call.
void ThrowIfFailed(gprx_status st, gprx_ctx* ctx);

template <class TScalarType>
class GaussianProcess {
public:
    typedef GaussianProcess Self;
    typedef std::shared_ptr<Self> Pointer;
    typedef Kernel<TScalarType> KernelType;
    typedef typename KernelType::Pointer KernelTypePointer;
    typedef DenseVector<TScalarType> VectorType;
    typedef DenseMatrix<TScalarType> MatrixType;
    typedef std::vector<VectorType> VectorListType;
    typedef long double HighPrecisionType;
    typedef enum { FullPivotLU = 0, JacobiSVD = 1, BDCSVD = 2, SelfAdjointEigenSolver = 3 } InversionMethod;

    explicit GaussianProcess(KernelTypePointer kernel);
    virtual ~GaussianProcess();
    GaussianProcess(const Self&) = delete;
    void operator=(const Self&) = delete;

    void AddSample(const VectorType& x, const VectorType& y);
    // Erases sample `index` and its label (throws when there is none).  A sample that is resident
    // on the device is queued for Update(), which takes it out of the device factor
    // (gprx_model_remove) instead of refitting; Initialize() refits as always.  Not in the reference.
    void RemoveSample(std::size_t index);
    virtual VectorType Predict(const VectorType& x);
    virtual VectorType PredictDerivative(const VectorType& x, MatrixType& D);
    virtual TScalarType operator()(const VectorType& x, const VectorType& y);
    TScalarType GetCredibleInterval(const VectorType& x);
    virtual void Initialize();
    // Initialize() for a GP that only GREW or SHRANK since its last device fit: when the device
    // holds a Cholesky factor made with the current kernel and sigma and the only changes since are
    // RemoveSample and AddSample calls, the queued removals are applied to that factor in order
    // (gprx_model_remove), then the samples added since extend it (gprx_model_append, O(N^2 c)),
    // instead of the O(N^3) refit; in every other state this is Initialize().  Opt-in:
    // Initialize() and the calls that imply it always refit.  Not in the reference.
    virtual void Update();

    // Batched, device-native forms (one launch for all rows; not in the reference).
    MatrixType PredictBatch(const MatrixType& Xq);                 // rows = queries -> q x m
    std::vector<TScalarType> CredibleIntervalBatch(const MatrixType& Xq);

    const KernelTypePointer GetKernel() { return m_Kernel; }
    void SetKernel(KernelTypePointer k) {
        m_Kernel = k;
        m_Initialized = false;
    }
    void DebugOn() { debug = true; }
    virtual unsigned GetNumberOfSamples() const { return (unsigned)m_SampleVectors.size(); }
    TScalarType GetSigma() const { return m_Sigma; }
    TScalarType GetSigmaSquared() const { return m_Sigma * m_Sigma; }
    void SetSigma(TScalarType sigma) {
        m_Sigma = sigma;
        m_Initialized = false;
    }
    // Per-dimension length scales (gprx_model_set_length_scales; not in the reference, whose kernels
    // are isotropic): the GP's kernel becomes k(x / ell, y / ell), one metric for every leaf of the
    // kernel tree.  An empty vector clears them.  Checked against the input dimension (and refused for
    // a kernel with no device form) when the state next goes to the device.  Save refuses a GP with
    // length scales: the reference's five files have no place for them.
    void SetLengthScales(const VectorType& ell) {
        m_LengthScales = ell;
        m_ScalesUploaded = false;
        m_Initialized = false;
        m_DeviceFactor = false;
        m_FitCholesky = false;
    }
    const VectorType& GetLengthScales() const { return m_LengthScales; }
    virtual unsigned GetNumberOfInputDimensions() const { return m_InputDimension; }
    virtual void SetInversionMethod(InversionMethod m) { m_InvMethod = m; }
    virtual InversionMethod GetInversionMethod() { return m_InvMethod; }
    bool GetEfficientStorage() { return m_EfficientStorage; }
    void SetEfficientStorage(bool s) { m_EfficientStorage = s; }

    virtual void Save(std::string prefix);
    virtual void Load(std::string prefix);
    virtual void ToString() const;

    void Lock() { gp_lock.lock(); }
    void UnLock() { gp_lock.unlock(); }

    virtual bool operator==(const GaussianProcess<TScalarType>& b) const;
    virtual bool operator!=(const GaussianProcess<TScalarType>& b) const { return !operator==(b); }

    // The explicit core matrix (K + sigma^2 I)^{-1}, materialised from the device factor.
    const MatrixType& GetCoreMatrix();

    // Leave-one-out cross-validation (gprx_model_loo; not in the reference): every sample's mean
    // (n x m) and variance (n) predicted from all the others, from the device's Cholesky factor
    // without refitting.  Returns the predictive log probability summed over the outputs.
    TScalarType LeaveOneOut(MatrixType& mean, VectorType& variance);

    // The JOINT posterior over the points xs (gprx_model_posterior; not in the reference, whose
    // operator() gives one pair): mean (q x m, what Predict returns per point) and the full q x q
    // covariance, from the device's Cholesky factor without refitting.  noise: sigma^2 added to the
    // diagonal (the distribution of observations instead of the latent function).
    void GetPosterior(const std::vector<VectorType>& xs, MatrixType& mean, MatrixType& cov, bool noise = false);
    // nsamples joint draws at xs (gprx_model_sample): each a q x m matrix, mean + Lq z with Lq the
    // Cholesky factor of that covariance (plus the automatic jitter) and z from the device's
    // counter-based normal generator keyed by `seed`; draw i does not depend on nsamples.
    std::vector<MatrixType> Sample(const std::vector<VectorType>& xs, std::size_t nsamples, uint64_t seed,
                                   bool noise = false);

protected:
    KernelTypePointer m_Kernel;
    TScalarType m_Sigma;
    VectorListType m_SampleVectors;
    VectorListType m_LabelVectors;
    MatrixType m_RegressionVectors;
    MatrixType m_CoreMatrix;
    bool m_Initialized;
    unsigned m_InputDimension;
    unsigned m_OutputDimension;
    InversionMethod m_InvMethod;
    bool m_EfficientStorage;
    std::mutex gp_lock;
    bool debug;

    gprx_model* m_Model = nullptr;
    std::mutex m_DevMu;           // guards the lazy refit (EnsureFactor), m_CoreMatrix/m_CoreSize
    bool m_DeviceFactor = false;  // device holds the Cholesky factor of the current state
    bool m_HostKernel = false;    // the kernel has no device form (Describe throws): K and the
                                  // kernel vectors are evaluated here through the virtual
                                  // operator() (include/Kernel.h:52-59), the rest on the device
    bool m_CoreValid = false;     // m_CoreMatrix holds the materialised core matrix
    bool m_DataUploaded = false;  // the device model holds the first m_DeviceSamples samples as
                                  // they are here: an optimiser loop re-evaluating the likelihood
                                  // under new kernel parameters re-sends only the kernel, and
                                  // Update() only the samples added since
    VectorType m_LengthScales;        // per-dimension length scales, empty: none
    bool m_ScalesUploaded = true;     // the device model holds m_LengthScales (UploadState sends them)
    std::size_t m_DeviceSamples = 0;  // samples resident on the device (UploadState re-sends all
                                      // of them when it differs from the sample count)
    // RemoveSample calls on device-resident samples since the device data was last in step: the
    // index each had on the device once the earlier ones are applied (Update applies them in order;
    // UploadState re-sends everything instead)
    std::vector<std::size_t> m_PendingRemovals;
    // the device factor's provenance (FitDevice, Update): a Cholesky factor, and the kernel and
    // sigma it was made with -- Update() extends it only while these still hold
    bool m_FitCholesky = false;
    std::string m_FitKernel;
    TScalarType m_FitSigma = 0;
    std::size_t m_CoreSize = 0;   // the reference's m_CoreMatrix.diagonalSize(): n once the
                                  // core exists (Initialize w/o efficient storage, operator(),
                                  // Load), 0 when efficient storage dropped it

    void CheckInputDimension(const VectorType& x, std::string msg_prefix) const;
    void CheckOutputDimension(const VectorType& y, std::string msg_prefix) const;
    gprx_model* Model();
    void UploadState();            // samples, kernel, noise -> device
    void FitDevice(gprx_fit_info* info = nullptr);
    void EnsureFactor();           // factor for operator()/core; keeps the regression vectors
                                   // (caller holds m_DevMu)
    // host-evaluated kernel rows K(x, X) of q queries (rows of Xq, or one vector), row-major
    std::vector<TScalarType> HostKernelRows(const TScalarType* Xq, std::size_t q) const;
    std::vector<TScalarType> HostDerivativeMatrices(int32_t& P) const;  // P x n x n

    friend class Likelihood<TScalarType>;
};

}  // namespace gpr
