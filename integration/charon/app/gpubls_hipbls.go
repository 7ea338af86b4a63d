//go:build hipbls

package app

import (
	"context"

	"github.com/obolnetwork/charon/app/log"
	"github.com/obolnetwork/charon/app/z"
	"github.com/obolnetwork/charon/tbls"
	"github.com/obolnetwork/charon/tbls/hipbls"
)

// selectGPUBLS binds libhipbls to every GPU of the node (one charon process per node drives them all, one device
// context each) and installs it as the tbls implementation.  parsigex and sigagg then take their batch paths
// (wireCoreWorkflow type-asserts tbls.BatchVerifier).
func selectGPUBLS(ctx context.Context) error {
	impl, err := hipbls.New()
	if err != nil {
		return err
	}
	// The resident H(m) cache: a signing root is hashed to G2 when its first partials are verified (parsigex,
	// validatorapi) and read again by every later batch of that root and by sigagg.
	if err := hipbls.ConfigHCache(hipbls.DefaultHCacheCapacity); err != nil {
		return err
	}
	// The signature cache (hipbls.ConfigSigCache, hipbls.DefaultSigCacheSlots) stays off: sigagg alone gains 9 % (wire)
	// and 23 % (keyed) from it, but over the whole flow, parsigex's Verify of every partial and then sigagg, the gain
	// was below five times the run-to-run spread (DESIGN.md 4.14).
	tbls.SetImplementation(impl)
	log.Info(ctx, "tbls backed by the GPU implementation", z.Str("impl", "hipbls"))

	return nil
}
