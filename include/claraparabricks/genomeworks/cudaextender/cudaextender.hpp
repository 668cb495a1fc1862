// cudaextender.hpp -- status codes and extension kinds of the cudaextender library (libcudaextender.so).
#pragma once

namespace claraparabricks
{
namespace genomeworks
{
namespace cudaextender
{

/// Result of an Extender call.
enum StatusType
{
    success           = 0, ///< done
    invalid_operation = 1, ///< call not valid in the object's current state (e.g. sync() without a host-pointer extend)
    invalid_input     = 2, ///< null pointer, negative length or count
    generic_error          ///< anything else (device error)
};

/// Kind of extension an Extender performs. Only ungapped X-drop exists.
enum ExtensionType
{
    ungapped_xdrop = 0,
};

/// Library initialisation (sets up logging). Returns success.
StatusType Init();

} // namespace cudaextender
} // namespace genomeworks
} // namespace claraparabricks
